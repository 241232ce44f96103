"""References, operand builders, bounds and case tables of tests/test_image_side_ops_gpu.py: the two image-side layers
(rna_gan_amd/csrc/rg_skinny.hip, their generic routes in rg_generic.hip, the dispatch in rg_api.hip) and the critic head kernels
(rg_misc.hip), pinned on the CPU by tests/test_image_side_refs_cpu.py.  No GPU here; every function runs on the device of its
arguments, and operands are drawn from a CPU torch.Generator with fixed seeds, so both test files see the same numbers.

A  EXACT INTEGERS.  Images and low-resolution activations hold {-2, -1, +1, +2} (dense), weights {-1, 0, +1}, biases small
   integers, slopes 0.5 and 1; the fused BatchNorm has an integer mean, invstd * gamma in {0.5, 1, 2} and an integer beta; tb_img
   holds {0, +-0.5, +-1} (1 - img^2 in {1, 0.75, 0}); sign-bit masks come from an activation holding +1, -1, +0, -0.  Every
   product and every partial sum in any order is then an fp32 number (S = sum |a||b| <= 2^24, asserted), so an fp32 output
   must equal the reference and a 16-bit output the reference rounded once to the storage type (C1 of
   tests/test_ops_exact_gpu.py states the argument; its matrix-product references are reused here).
B  GAUSSIAN OPERANDS against fp64 under |got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25 (`bound`), u from UNIT.
   tanh: TANH_RECIPE_BOUND is derived below from the recipe of the row kernels, TANH_LIBM_ULPS is what the vector kernels get.

The dispatch is mirrored by kernel_first_down / kernel_last_up / kernel_wgrad: every case of the tables names the kernel it takes,
and the GPU tests check the mirror against what the library's own queries tell (rg_first_down_masked_supported,
rg_last_up_post_blocks, the slab count of rg_skinny_wgrad_slabs).
"""
import collections
import itertools

import torch

from test_ops_exact_gpu import ref_down, ref_up, ref_wgrad

I = 3
K_DOWN = 16 * I
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}      # unit round-off of a storage type
SLOPE, MSLOPE = 0.5, 0.5
L32 = 2.0 ** 24
SK_ROWS_BLOCKS, LU_BLOCKS, W128_BLOCKS = 768, 512, 512              # grid caps of the row kernels (rg_skinny.hip)

# --------------------------------------------------------------------------------------------------------------- the cases
# (N, Ho, Wo) are the low-resolution dimensions: the image is [N, 3, 2 Ho, 2 Wo], the activation [N, Ho, Wo, O].
# ops: which of first_down ("d"), last_up ("u"), the weight gradient ("w") run the case.
Case = collections.namedtuple("Case", "name N Ho Wo O storage ops why")
CASES = [
    # general row kernels, one unit per row, one per chunk size
    Case("row32_h2", 1, 1, 32, 64, "h16", "duw", "H = 2: top and bottom padding in the same unit; one strip of one row"),
    Case("row64", 2, 3, 64, 64, "h16", "duw", "chunk 64, 6 units, strips of 3"),
    Case("row128", 1, 5, 128, 64, "h16", "duw", "chunk 128, 5 units, one strip of 5"),
    # two and three chunks per row: the edge lanes / halo pixels read a real neighbour column
    Case("seam2", 1, 3, 256, 64, "h16", "duw", "cpr = 2"),
    Case("seam3", 2, 2, 384, 64, "h16", "duw", "cpr = 3: a chunk with a neighbour on both sides"),
    # strips of last_up
    Case("strips2", 1, 32, 32, 64, "h16", "duw", "Ho = 32: two strips of 16 per image"),
    Case("strips10", 1, 20, 32, 64, "h16", "u", "Ho = 20: strips of 10"),
    Case("strips1", 1, 17, 32, 64, "h16", "u", "Ho = 17 (prime): strips of one row, the ring refilled for every row"),
    Case("strips12", 2, 24, 64, 64, "h16", "u", "strips of 12, two images"),
    # work lists longer than the grid
    Case("units775", 5, 155, 32, 64, "h16", "dw", "775 units on 768 blocks: per = 2, the last working block holds one unit"),
    Case("strips565", 5, 113, 32, 64, "h16", "u", "565 strips of one row on 512 blocks"),
    # 256 x 256 images: the rows128 kernels (option skinny128 = 1) and the general ones (= 0)
    Case("r128_n1", 1, 128, 128, 64, "h16", "duw", "128 units, 8 strips"),
    Case("r128_n5", 5, 128, 128, 64, "h16", "w", "640 units on the 512 blocks of skinny_wgrad_rows128_kernel"),
    Case("r128_n7", 7, 128, 128, 64, "h16", "duw", "896 units on 768 blocks, 56 strips"),
    # vector and generic routes through the same entry points
    Case("o4", 2, 4, 32, 4, "h16", "duw", "O = 4: not rg_skinny_supported, the generic GEMM"),
    Case("o32", 2, 4, 32, 32, "h16", "duw", "O = 32: the generic GEMM"),
    Case("o128", 2, 4, 32, 128, "h16", "duw", "O = 128: the vector kernels of rg_skinny.hip"),
    Case("w16", 2, 3, 16, 64, "h16", "duw", "Wo = 16 has no chunk: vector kernels"),
    Case("w48", 1, 3, 48, 64, "h16", "duw", "Wo = 48 has no chunk: vector kernels"),
    Case("f32_o4", 2, 4, 32, 4, "f32", "duw", "fp32 storage, generic"),
    Case("f32_o64", 2, 4, 32, 64, "f32", "duw", "fp32 storage, powers of two: rg_generic_f32_image_side with f32mma != 0"),
    Case("f32_o128", 2, 4, 32, 128, "f32", "duw", "the same at O = 128"),
    Case("f32_o64_np2", 1, 3, 48, 64, "f32", "duw", "fails rg_generic_f32_image_side (3 x 48): the vector kernels whatever f32mma"),
]
BY_NAME = {c.name: c for c in CASES}
LARGE = ("r128_n5", "r128_n7")                    # the CPU test checks only operand ranges and S bounds of these


def cases(op):
    return [c for c in CASES if op in c.ops]


def chunk_of(Wo):
    """sk_rows_chunk: the unit width of the row kernels, None where there is none"""
    if Wo >= 128 and Wo % 128 == 0:
        return 128
    return Wo if Wo in (32, 64) else None


def skinny(O):
    return O % 64 == 0 and O <= 128               # rg_skinny_supported (I = 3)


def rows(c):
    """the matrix-core row kernels take the case (16-bit storage, 64 channels, a chunk)"""
    return c.storage == "h16" and c.O == 64 and chunk_of(c.Wo) is not None


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def f32_generic(c, f32mma):
    """rg_generic_f32_image_side; MB_K is a build-time 16 or 32 -- the tables use Wo = 32 (passes both) and Wo = 48 (fails both)"""
    assert c.Wo >= 32
    return f32mma != 0 and _pow2(c.Ho) and _pow2(c.Wo) and c.O >= 33 and c.N * c.Ho * c.Wo >= 64


def variants(c):
    """the option settings under which a case runs (through _Options): both kinds of row kernel at 256 x 256, both sides of
    rg_generic_f32_image_side on fp32 storage"""
    if rows(c) and (c.Ho, c.Wo) == (128, 128):
        return [{"skinny128": 1}, {"skinny128": 0}]
    if c.storage == "f32" and skinny(c.O):
        return [{"f32mma": 0}, {"f32mma": 1}, {"f32mma": 2}]
    return [{}]


def _r128(c, opts):
    return (c.Ho, c.Wo) == (128, 128) and opts.get("skinny128", 1) != 0


def kernel_first_down(c, opts):
    if rows(c):
        return "first_down_rows128_kernel" if _r128(c, opts) else "first_down_rows_kernel"
    if not skinny(c.O):
        return "rg_generic_first_down"
    if c.storage == "f32":
        return "rg_generic_first_down" if f32_generic(c, opts.get("f32mma", 2)) else "first_down_kernel<float>"
    return "first_down_kernel<h16>"


def kernel_last_up(c, opts):
    if rows(c):
        return "last_up_rows128_kernel" if _r128(c, opts) else "last_up_rows_kernel"
    if not skinny(c.O):
        return "rg_generic_last_up"
    return "last_up_kernel<float, 4, 16>" if c.storage == "f32" else "last_up_kernel<h16, 8>"


def kernel_wgrad(c, opts):
    if rows(c):
        return "skinny_wgrad_rows128_kernel" if _r128(c, opts) else "skinny_wgrad_rows_kernel"
    if not skinny(c.O):
        return "rg_generic_skinny_wgrad"
    if c.storage == "f32":
        return "rg_generic_skinny_wgrad" if f32_generic(c, opts.get("f32mma", 2)) else "skinny_wgrad_kernel<float>"
    return "skinny_wgrad_kernel<h16>"


def units(c):
    return c.N * c.Ho * c.Wo // chunk_of(c.Wo)


def strip_of(Ho):
    s = min(Ho, 16)
    while Ho % s:
        s -= 1
    return s


def strips(c):
    return c.N * (c.Ho // strip_of(c.Ho)) * (c.Wo // chunk_of(c.Wo))


def post_blocks(c):
    return min(strips(c), LU_BLOCKS) if rows(c) else 0


def wgrad_slabs(c, opts):
    """*nslab_out of rg_skinny_wgrad_slabs (0: no slab form)"""
    if not rows(c):
        return 0
    n = min(units(c), SK_ROWS_BLOCKS)
    return min(n, W128_BLOCKS) if _r128(c, opts) else n


# ------------------------------------------------------------------------------------------------------------- the operands
def ints12(shape, gen):
    """dense {-2, -1, +1, +2} (as _ints12 of tests/test_ops_exact_gpu.py, drawn on the CPU)"""
    r = torch.randint(0, 4, shape, generator=gen)
    return (r % 2 + 1).float() * (1 - 2 * (r // 2)).float()


def ints01(shape, gen):
    return (torch.randint(0, 3, shape, generator=gen) - 1).float()


def signed_zeros(shape, gen):
    """+1, -1, +0, -0 in equal parts: zero of either sign is "not positive" """
    r = torch.randint(0, 4, shape, generator=gen)
    return torch.tensor([1.0, -1.0, 0.0, -0.0])[r]


def tb_values(shape, gen):
    """{0, +-0.5, +-1}: +-1 (factor 0) for 1/16 of the pixels, so that the zero outputs stay below 10 %"""
    r = torch.randint(0, 32, shape, generator=gen)
    table = torch.tensor([1.0, -1.0] + [0.0] * 10 + [0.5] * 10 + [-0.5] * 10)
    return table[r]


def operands(c):
    """every operand of a case, fp32 on the CPU (the values are exact in bf16 and fp16):
    x [N, 3, H, W], w [O, 3, 4, 4] (torch layout, both layers), bd [O] / bu [3] the biases, a [N, Ho, Wo, O] the low-resolution
    activation (input of last_up, `low` of the weight gradient), m the activation whose sign bits mask first_down, mean / invstd /
    gamma / beta of the fused BatchNorm (BN(0) != 0 in every channel), tb the tanh image of rg_last_up_post."""
    gen = torch.Generator().manual_seed(4200 + CASES.index(c))
    N, Ho, Wo, O = c.N, c.Ho, c.Wo, c.O
    p = {"x": ints12((N, I, 2 * Ho, 2 * Wo), gen), "w": ints01((O, I, 4, 4), gen),
         "bd": torch.randint(-3, 4, (O,), generator=gen).float(), "bu": torch.tensor([-3.0, 1.0, 2.0]),
         "a": ints12((N, Ho, Wo, O), gen)}
    if c.O == 64 and c.storage == "h16":
        p["m"] = signed_zeros((N, Ho, Wo, O), gen)
    if rows(c):
        p["mean"] = torch.randint(-2, 3, (O,), generator=gen).float()
        p["invstd"] = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (O,), generator=gen)]
        p["gamma"] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (O,), generator=gen)]
        beta = torch.randint(-3, 4, (O,), generator=gen).float()
        bn0 = beta - p["mean"] * p["invstd"] * p["gamma"]
        p["beta"] = torch.where(bn0 == 0, beta + 1, beta)             # BN(0) != 0: padding that passed through bn8 would show
        p["tb"] = tb_values((N, I, 2 * Ho, 2 * Wo), gen)
    return p


def gauss_operands(c):
    """part B: x, w (std 0.2), a Gaussian, as fp32; the 16-bit `a` is rounded by the caller"""
    gen = torch.Generator().manual_seed(9100 + CASES.index(c))
    return {"x": torch.randn((c.N, I, 2 * c.Ho, 2 * c.Wo), generator=gen), "w": torch.randn((c.O, I, 4, 4), generator=gen) * 0.2,
            "a": torch.randn((c.N, c.Ho, c.Wo, c.O), generator=gen)}


# ----------------------------------------------------------------------------------------------------------- the references
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def ohwi(w):
    return w.permute(0, 2, 3, 1).contiguous()


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def first_down(x, w, bias=None, slope=1.0, factor=None):
    """x [N, 3, H, W], w [O, 3, 4, 4] -> lrelu(conv2d(x, w, stride 2, pad 1) + bias) [* factor], NHWC"""
    y = ref_down(nhwc(x), ohwi(w))
    if bias is not None:
        y = y + bias
    y = lrelu(y, slope)
    return y if factor is None else y * factor


def last_up(a, w, bias=None):
    """a [N, Ho, Wo, O], w [O, 3, 4, 4] -> conv_transpose2d(a, w, stride 2, pad 1) + bias, NCHW"""
    y = ref_up(a, ohwi(w)).permute(0, 3, 1, 2).contiguous()
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def wgrad(low, x):
    """low [N, Ho, Wo, O], x [N, 3, H, W] -> the gradient of first_down's weight [O, 3, 4, 4]"""
    return ref_wgrad(low, nhwc(x)).permute(0, 3, 1, 2).contiguous()


def wgrad_live(c, device="cpu"):
    """[3, 4, 4] mask of the taps that meet at least one pixel inside the image (H = 2: rows kh = 0 and kh = 3 only ever see padding)"""
    one = torch.ones(1, I, 2 * c.Ho, 2 * c.Wo, device=device)
    return wgrad(torch.ones(1, c.Ho, c.Wo, 1, device=device), one)[0] > 0


def bn_act(z, mean, invstd, gamma, beta, slope):
    return lrelu((z - mean) * (invstd * gamma) + beta, slope)


def mask_factor(m, mslope):
    return torch.where(m > 0, 1.0, mslope).to(m.dtype)


def sign_words(y):
    """[..., 64] -> int64 words, bit c = (y[..., c] > 0)"""
    assert y.shape[-1] == 64
    sh = torch.arange(64, device=y.device)
    return ((y > 0).long() << sh).sum(-1)


def words_hold_both_values(words):
    """every one of the 64 bit positions is 1 somewhere and 0 somewhere"""
    w = words.reshape(-1)
    sh = torch.arange(64, device=w.device)
    b = (w[:, None] >> sh) & 1
    return bool(b.any(0).all()) and bool((b == 0).any(0).all())


def post_sums(v):
    """v [N, 3, H, W] (fp64) -> [4]: the three channel sums and the sum of squares (the columns of rg_last_up_post's partial rows)"""
    return torch.cat([v.sum((0, 2, 3)), (v * v).sum().view(1)])


# ----------------------------------------------------------------------------------------------------------- the conditions
def conditions(ref, S, what, live=None, terms=None):
    """Asserted on the reference alone, before any comparison.  S <= 2^24; at most 10 % of the outputs zero; at least 50 distinct
    values.  Where arithmetic rules the 50 out, fewer are asked, never less than "not a constant":
      - an output of n entries is asked for n // 4 (a bias gradient has 64 entries); one of fewer than 50 entries only has to be
        no constant;
      - `terms`: an output that sums that many products of {+-1, +-2} x {-1, 0, +1} has the standard deviation
        sigma = sqrt(terms * 5/2 * 2/3), and a sample shows the integers within about +-3 sigma: 50 of them need terms >= 42.
        first_down at H = 2 has 24 terms (two of four kernel rows are padding), last_up at O = 4 has 16: they are asked for the
        integers within +-2 sigma, 4 sigma values;
      - `live` excludes entries that are structurally zero (weight-gradient taps that only meet padding)."""
    assert float(S.max()) <= L32, "%s: S = %g > 2^24: not every partial sum is exact" % (what, float(S.max()))
    r = ref if live is None else ref[live.expand_as(ref)]
    zeros = float((r == 0).float().mean())
    distinct = int(torch.unique(r).numel())
    need = min(50, max(2, r.numel() // 4))
    if r.numel() < 50:
        assert distinct >= 2, "%s: a constant" % what
        return
    if terms is not None:
        need = min(need, int(4 * (terms * 5 / 3) ** 0.5))
    assert zeros <= 0.10 and distinct >= need, "%s: trivial case (%.1f %% zeros, %d distinct values of %d asked)" % (
        what, 100 * zeros, distinct, need)
    if live is not None:
        assert bool((ref[~live.expand_as(ref)] == 0).all())


def down_refs(c, p):
    """every expected first_down output of a case (fp32 values; a 16-bit build stores them rounded once), conditions asserted:
    plain = slope 0.5 with bias, lin = slope 1 without, masked = lin x (mask bit ? 1 : 0.5), the sign-bit words of plain and of m"""
    x, w = p["x"], p["w"]
    S = first_down(x.abs(), w.abs(), p["bd"].abs())
    r = {"plain": first_down(x, w, p["bd"], SLOPE), "lin": first_down(x, w)}
    terms = K_DOWN // 2 if c.Ho == 1 else K_DOWN
    conditions(r["plain"], S, c.name + " first_down", terms=terms)
    conditions(r["lin"], S, c.name + " first_down (slope 1, no bias)", terms=terms)
    assert float(r["plain"].abs().max()) < 128 and float(r["lin"].abs().max()) < 128       # halves below 128: 8 significant bits
    if "m" in p:
        r["masked"] = r["lin"] * mask_factor(p["m"], MSLOPE)
        conditions(r["masked"], S, c.name + " first_down_masked", terms=terms)
        r["m_words"], r["plain_words"] = sign_words(p["m"]), sign_words(r["plain"])
        assert words_hold_both_values(r["m_words"]) and words_hold_both_values(r["plain_words"]), c.name + ": a constant sign bit"
    return r


def strip_region(c, sidx):
    """(n, first low-resolution row, rows, first low-resolution column, columns) of strip sidx of the last_up row kernels"""
    chunk, strip = chunk_of(c.Wo), strip_of(c.Ho)
    cpr, spi = c.Wo // chunk, c.Ho // strip
    cx, rest = sidx % cpr, sidx // cpr
    return rest // spi, (rest % spi) * strip, strip, cx * chunk, chunk


def post_rows(c, v):
    """v [N, 3, H, W] -> [blocks, 4], the partial rows of rg_last_up_post: workgroup b sums the strips b, b + blocks, ..."""
    nb = post_blocks(c)
    rows_ = torch.zeros(nb, 4, dtype=torch.float64, device=v.device)
    v = v.double()
    for sidx in range(strips(c)):
        n, h0, sh, w0, sw = strip_region(c, sidx)
        rows_[sidx % nb] += post_sums(v[n:n + 1, :, 2 * h0:2 * (h0 + sh), 2 * w0:2 * (w0 + sw)])
    return rows_


def up_refs(c, p):
    """every expected last_up output (NCHW fp32), conditions asserted: plain, bias; for the row kernels pre (the fused BatchNorm +
    LeakyReLU of the input, `act` being what rg_bn_act would store), post_tb (x 1 - tb^2), zero (the first strip of every image's
    input zeroed: no conditions, the whole output of a one-strip case is then zero)"""
    a, w = p["a"], p["w"]
    S = last_up(a.abs(), w.abs(), p["bu"].abs())
    r = {"plain": last_up(a, w), "bias": last_up(a, w, p["bu"])}
    conditions(r["plain"], S, c.name + " last_up", terms=4 * c.O)
    conditions(r["bias"], S, c.name + " last_up (bias)", terms=4 * c.O)
    if rows(c):
        act = bn_act(a, p["mean"], p["invstd"], p["gamma"], p["beta"], SLOPE)
        assert float(act.abs().max()) <= 16 and torch.equal(4 * act, (4 * act).round()), "the activation is a 16-bit number (6 bits)"
        bn0 = bn_act(torch.zeros(c.O, device=a.device), p["mean"], p["invstd"], p["gamma"], p["beta"], SLOPE)
        assert bool((bn0 != 0).all()), "BN(0) != 0 in every channel"
        r["act"], r["pre"] = act, last_up(act, w, p["bu"])
        conditions(r["pre"], last_up(act.abs(), w.abs(), p["bu"].abs()), c.name + " last_up_pre")
        assert in_set(p["tb"], [0.0, 0.5, -0.5, 1.0, -1.0])
        r["post_tb"] = r["plain"] * (1 - p["tb"] * p["tb"])
        conditions(r["post_tb"], S, c.name + " last_up_post (tanh backward)")
        a0 = a.clone()
        a0[:, :strip_of(c.Ho)] = 0
        r["a_zero"], r["zero"] = a0, last_up(a0, w)
    return r


def wgrad_refs(c, p):
    """dw [O, 3, 4, 4] and the bias gradient [O] = the column sums of `low`"""
    a, x = p["a"], p["x"]
    r = {"dw": wgrad(a, x), "db": a.reshape(-1, c.O).sum(0)}
    conditions(r["dw"], 2 * wgrad(a.abs(), x.abs()), c.name + " skinny_wgrad (accumulated once)", live=wgrad_live(c, a.device))
    conditions(r["db"], 2 * a.abs().reshape(-1, c.O).sum(0), c.name + " bias gradient")
    return r


def operand_ranges(c, p):
    """the integer ranges of part A and S <= 2^24 by counting alone (what the CPU test asserts of the largest cases)"""
    assert in_set(p["x"], [-2.0, -1.0, 1.0, 2.0]) and in_set(p["a"], [-2.0, -1.0, 1.0, 2.0]) and in_set(p["w"], [-1.0, 0.0, 1.0])
    assert torch.equal(p["bd"], p["bd"].round()) and torch.equal(p["bu"], p["bu"].round()) and float(p["bd"].abs().max()) <= 3
    assert 2 * (K_DOWN * 2 + 3) <= L32 and 2 * (4 * c.O * 2 + 3) <= L32                  # first_down, last_up
    assert 2 * 4 * c.N * c.Ho * c.Wo <= L32                                              # the weight gradient, accumulated once
    if "m" in p:
        assert in_set(p["m"], [1.0, -1.0, 0.0]) and bool((p["m"] == 0).any()) and bool(torch.signbit(p["m"][p["m"] == 0]).any())
        assert bool((~torch.signbit(p["m"][p["m"] == 0])).any())
    if rows(c):
        scale = p["invstd"] * p["gamma"]
        assert in_set(scale, [0.5, 1.0, 2.0]) and torch.equal(p["mean"], p["mean"].round()) and torch.equal(p["beta"], p["beta"].round())
        assert in_set(p["tb"], [0.0, 0.5, -0.5, 1.0, -1.0])


def in_set(t, values):
    return bool(torch.isin(t, torch.tensor(values, dtype=t.dtype, device=t.device)).all())


def bound(ref, S, K, u):
    """|got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25: K fp32 roundings along a sum whose terms have magnitudes summing to S, one
    rounding to the stored type (u = 0: an fp32 result).  Nothing in it is measured."""
    return u * ref.abs() + K * 2.0 ** -24 * (1 + u) * S + 2.0 ** -25


# ----------------------------------------------------------------------------------------------------------------- tanh
# last_up_rows_kernel / last_up_rows128_kernel evaluate tanh(x) = 1 - 2 rcp(exp2(x c) + 1), c = fl(2 log2 e), in fp32:
#   t = fl(x c)       c carries a relative 2^-24 and the product another: |dt| <= 2^-23 |t|.  With y = 2 x,
#                     out = tanh(y / 2), d out / d y = 2 e / (e + 1)^2 (e = exp y) and dy / y = dt / t:
#                     |d out| <= 2^-23 * sup_y |2 y e / (e + 1)^2| = 2^-23 * 0.4478 (at |y| = 1.5434).
#   e = exp2(t)       v_exp_f32: 1 ulp, a relative 2^-23;  |d out| = 2 e / (e + 1)^2 * 2^-23 <= 2^-23 / 2  (e / (e + 1)^2 <= 1/4).
#   s = fl(e + 1)     a relative 2^-24 of s;  out = 1 - 2 / s, |d out| = 2 / s * 2^-24 <= 2^-23  (s >= 1).
#   r = rcp(s)        v_rcp_f32: 1 ulp, a relative 2^-23 of r <= 1;  |d out| = 2 r 2^-23 <= 2 * 2^-23.
#   out = fl(1 - 2 r) 2 r is exact; |out| <= 1: at most 2^-24.
# In sum 2^-23 (0.4478 + 0.5 + 1 + 2) + 2^-24 = 4.448 * 2^-23; second-order terms are below 2^-40.  (exp2 saturates to 0 / inf
# outside |x| > 44, where the recipe returns -1 / +1 and tanh is within 2^-120 of that.)
TANH_RECIPE_BOUND = 4.5 * 2.0 ** -23             # absolute; 5.4e-7
TANH_LIBM_ULPS = 2.0                             # the vector kernels call tanhf: 2 ulp of the result, |err| <= 2 * 2^-23 |tanh x|
TANH_C = 2.885390081777927                       # the kernels' constant


def tanh_recipe(x, signs):
    """the recipe in fp64 with every step pushed by its unit in the direction signs[k] (each +-1): (t, e, s, r, out)"""
    c32 = float(torch.tensor(TANH_C, dtype=torch.float32))
    t = x * c32 * (1 + signs[0] * 2.0 ** -24)
    e = torch.exp2(t) * (1 + signs[1] * 2.0 ** -23)
    s = (e + 1) * (1 + signs[2] * 2.0 ** -24)
    r = (1 / s) * (1 + signs[3] * 2.0 ** -23)
    return (1 - 2 * r) + signs[4] * 2.0 ** -24


def tanh_sign_patterns():
    return list(itertools.product((-1.0, 1.0), repeat=5))


def tanh_bound(ref, libm):
    return TANH_LIBM_ULPS * 2.0 ** -23 * ref.abs() if libm else torch.full_like(ref, TANH_RECIPE_BOUND)


TANH_BIAS = torch.tensor([-21.0, 3.0, 40.0]) / 64      # k * 2^-6: integer sums + bias are fp32 numbers


# ----------------------------------------------------------------------------------------------------------------- head
# a [N][16][C] (tap-major), w [C][16] fp32, h[n] = sum_j a[n][j] wq[j] with j = tap C + c and wq[j] = w[c][tap]
HEAD_C = [6, 8, 264]                   # 264: the second trip of head_fwd's channel loop, a ragged last block of the weight gradients
HEAD_N = [1, 7, 9, 64]
HEAD_BIAS, HEAD_COEF = 3.0, 0.25


def head_operands(N, C):
    gen = torch.Generator().manual_seed(7000 + 300 * N + C)
    a, w = ints12((N, 16, C), gen), ints01((C, 16), gen)
    gh = torch.randint(-3, 4, (N,), generator=gen).float() * 0.25        # a small integer times a power of two
    gh[0] = 0.75
    return a, w, gh


def head_wq(w):
    return w.t().reshape(-1)                                            # [16 C], j = tap C + c


def head_fwd(a, w, bias, slope):
    h = a.reshape(a.shape[0], -1) @ head_wq(w)
    if bias is not None:
        h = h + bias
    return h, lrelu(h, slope)


def head_grad(h, coef, slope):
    return coef * torch.where(h > 0, 1.0, slope).to(h.dtype)


def head_bwd_data(gh, w):
    return gh[:, None] * head_wq(w)[None, :]                            # [N, 16 C]


def head_wgrad(gh, a):
    s = gh @ a.reshape(a.shape[0], -1)                                  # [16 C]
    return s.view(16, -1).t().contiguous()                              # dw[c][tap]


def head_h_values(N):
    """h for rg_head_grad: integers of both signs, +0 and -0 (zero is "not positive")"""
    gen = torch.Generator().manual_seed(7700 + N)
    h = torch.randint(-4, 5, (N,), generator=gen).float()
    h[0] = -0.0
    if N > 2:
        h[1], h[2] = 0.0, 5.0
    return h
