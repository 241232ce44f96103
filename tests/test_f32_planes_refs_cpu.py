"""(no GPU) tests/f32_planes_refs.py pinned against torch itself, and every condition of tests/test_f32_planes_ops_gpu.py checked
on the very operands the GPU tests use (fixed seeds, drawn on the CPU): the 2^8 / 2^7 / 2^24 bounds, the non-trivial-case rule
and "every (pair, k-tile) group is visible in every tile" -- so that a failing condition is found here and not on the GPU."""
import pytest
import torch
import torch.nn.functional as F

import f32_planes_refs as R


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def test_pair_tables_are_the_kernels():
    """hh hm mh hl lh mm as (A plane, B plane); the kernels decode pair pp from the nibbles of 0x120100 (A) and 0x102010 (B)
    (rg_conv8.hip decode, rg_wgrad8.hip flat_tile); the three-product tier is the first three."""
    assert R.PAIRS[6] == [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)] and R.PAIRS[3] == R.PAIRS[6][:3]
    assert R.PAIRS[6] == [((0x120100 >> (4 * pp)) & 15, (0x102010 >> (4 * pp)) & 15) for pp in range(6)]
    weights = [R.A_SCALE[p] * R.B_SCALE[q] for p in range(3) for q in range(3)]
    assert len(set(weights)) == 9 and min(weights) == 1 / R.UNIT                  # nine distinct powers of two down to 2^-16
    assert all(w * R.UNIT == round(w * R.UNIT) for w in weights)
    assert all(torch.tensor(s).bfloat16().item() == s for s in R.A_SCALE + R.B_SCALE)


@pytest.mark.parametrize("products", [6, 3])
def test_planes_expected_against_torch_convolutions(products):
    """fp64 conv2d / conv_transpose2d / conv2d_weight pair by pair: the sum of the convolutions of plane p of A with plane q
    of B over the pair set, i.e. the convolution of the summed operands restricted to that set"""
    gen = torch.Generator().manual_seed(3)
    for N, Hl, Wl, O, I in ((2, 4, 4, 5, 3), (1, 2, 6, 4, 6)):
        x = torch.randn(3, N, 2 * Hl, 2 * Wl, I, generator=gen, dtype=torch.float64)
        g = torch.randn(3, N, Hl, Wl, O, generator=gen, dtype=torch.float64)
        w = torch.randn(3, O, 4, 4, I, generator=gen, dtype=torch.float64)
        P = R.PAIRS[products]
        want = sum(F.conv2d(_nchw(x[p]), _nchw(w[q]), stride=2, padding=1).permute(0, 2, 3, 1) for p, q in P)
        assert torch.allclose(R.planes_expected("down", x, w, products), want, rtol=0, atol=1e-11)
        want = sum(F.conv_transpose2d(_nchw(g[p]), _nchw(w[q]), stride=2, padding=1).permute(0, 2, 3, 1) for p, q in P)
        assert torch.allclose(R.planes_expected("up", g, w, products), want, rtol=0, atol=1e-11)
        want = sum(torch.nn.grad.conv2d_weight(_nchw(x[q]), (O, I, 4, 4), _nchw(g[p]), stride=2, padding=1).permute(0, 2, 3, 1)
                   for p, q in P)
        assert torch.allclose(R.planes_expected("wgrad", g, x, products), want, rtol=0, atol=1e-11)
        # the full 3 x 3 product of the summed operands differs: the pair set matters
        full = F.conv2d(_nchw(x.sum(0)), _nchw(w.sum(0)), stride=2, padding=1).permute(0, 2, 3, 1)
        assert not torch.allclose(R.planes_expected("down", x, w, products), full, rtol=0, atol=1e-3)


def test_split_ref_against_integer_round_to_nearest_even():
    gen = torch.Generator().manual_seed(7)
    rnd = torch.randn(4096, generator=gen) * torch.exp(torch.randn(4096, generator=gen) * 8)
    v = torch.cat([R.structured_values(), rnd[rnd.abs() > 2.0 ** -100]])
    assert v.numel() == 7 + 228 * 7 * 2 + int((rnd.abs() > 2.0 ** -100).sum())
    pl = R.split_ref(v)
    assert pl.dtype == torch.bfloat16 and pl.shape == (3, v.numel())
    got = pl.view(torch.int16).to(torch.int32) & 0xffff
    fin = torch.isfinite(v)
    v64 = v.double()
    h = R.bf16_rne_bits(v64)
    hv = (h << 16).view(torch.float32).double()
    ok = fin & torch.isfinite(hv)                            # a magnitude that rounds to an infinite h: residual planes zero
    assert int((fin & ~ok).sum()) == 2 + 2 * 1               # +-3.4e38 and 2^127 x 1.7fffff, both signs
    assert torch.equal(got[0][fin], h[fin])
    r1 = torch.where(ok, v64 - hv, torch.zeros_like(v64))
    m = R.bf16_rne_bits(r1)
    r2 = r1 - (m << 16).view(torch.float32).double()
    assert torch.equal(r1.float().double(), r1) and torch.equal(r2.float().double(), r2)      # the residuals are fp32 numbers
    assert torch.equal(got[1][fin], m[fin]) and torch.equal(got[2][fin], R.bf16_rne_bits(r2)[fin])
    # v = h + m + l exactly; non-finite values keep their class in h with zero residuals
    s = pl.double().sum(0)
    assert torch.equal(s[ok], v64[ok])
    bad = ~ok
    assert not bool(torch.isfinite(pl[0].float()[bad]).any()) and bool((got[1][bad] == 0).all()) and bool((got[2][bad] == 0).all())
    assert bool(torch.isnan(pl[0].float()[4])) and float(pl[0][2]) == float("inf") and float(pl[0][3]) == float("-inf")
    assert int(got[0][0]) == 0 and int(got[0][1]) == 0x8000                                    # +0 and -0 keep their sign
    # the ties: 1.0 + 2^-8 rounds to even (down), 1.0 + 3 * 2^-8 rounds to even (up)
    t = torch.tensor([0x3f808000, 0x3f818000], dtype=torch.int32).view(torch.float32)
    assert (R.split_ref(t)[0].view(torch.int16).tolist()) == [0x3f80, 0x3f82]
    # outside the asserted set: the builder of the tiny values, whose residual planes can be subnormal
    tiny = R.tiny_values()
    assert float(tiny.abs().max()) < 2.0 ** -100 and tiny.numel() == 26 * 7 * 2 + 10
    assert R.tiled(v, 8).numel() == 8 and R.tiled(v, 2 ** 14 + 8).numel() == 2 ** 14 + 8


@pytest.mark.parametrize("kernel", list(R.PAIR_TABLE), ids=str)
def test_one_hot_conditions(kernel):
    """the operands of the pair-table test: bound and non-trivial case (asserted by the builder), and the expectation -- ref(X, W)
    for a pair of the tier, exactly zero otherwise -- is what planes_expected gives"""
    op, dims = R.KERNELS[kernel][0], R.PAIR_TABLE[kernel]
    for p in range(3):
        for q in range(3):
            A, B, ref = R.one_hot(op, dims, p, q)
            assert torch.equal(A.bfloat16().float(), A) and torch.equal(B.bfloat16().float(), B)
            for products in (6, 3) if kernel == "down256" else ():
                want = ref if (p, q) in R.PAIRS[products] else torch.zeros_like(ref)
                assert torch.equal(R.planes_expected(op, A, B, products), want)


@pytest.mark.parametrize("kernel,dims", R.SWEEP_CASES, ids=R.case_id)
def test_all_live_conditions_of_the_sweep(kernel, dims):
    op, bm, bn = R.KERNELS[kernel]
    A, B = R.sweep_operands(kernel, dims)
    assert torch.equal(A.bfloat16().float(), A) and torch.equal(B.bfloat16().float(), B)      # the planes are bf16 numbers
    for products in (6, 3):
        ref = R.live_reference(op, A, B, products, what=str(dims))
        assert torch.equal(ref.float().double(), ref)
        n = R.assert_conv_groups_live(op, A, B, products, bm, bn)
        assert n == products * 16 * (A.shape[-1] // 64)


@pytest.mark.parametrize("dims", R.MASK_CASES, ids=R.case_id)
def test_all_live_conditions_under_the_mask(dims):
    A, B, m, f = R.mask_operands(dims)
    z = m == 0
    neg0 = z & (m.view(torch.int32) < 0)
    assert bool((m > 0).any()) and bool((m < 0).any()) and bool(neg0.any()) and bool((z & ~neg0).any())
    assert bool((f[z] == R.SLOPE).all())                     # zero of either sign counts as "not positive"
    for products in (6, 3):
        ref = R.live_reference("up", A, B, products, L=R.L_MASK, factor=f, what="masked " + str(dims))
        assert torch.equal(ref.float().double(), ref)
        R.assert_conv_groups_live("up", A, B, products, 256, 64)


@pytest.mark.parametrize("kernel,dims,products", R.STATS_CASES, ids=R.case_id)
def test_unit_weight_conditions_of_the_statistics_cases(kernel, dims, products):
    op = R.KERNELS[kernel][0]
    A, B = R.stats_operands(kernel, dims, products)
    y, sums = R.unit_reference(op, A, B, products, what=kernel + str(dims))
    assert sums.shape == (2, y.shape[-1]) and torch.equal(sums.float().double(), sums)
    # the rows of the tail tile beyond M contribute nothing: the reference has exactly M (x 4 classes) rows
    N, Hl, Wl = dims[:3]
    assert y.reshape(-1, y.shape[-1]).shape[0] == N * Hl * Wl * (4 if op == "up" else 1) and (N * Hl * Wl) % R.KERNELS[kernel][1] != 0


@pytest.mark.parametrize("kernel,dims", R.WGRAD_CASES, ids=R.case_id)
def test_all_live_conditions_of_the_weight_gradient(kernel, dims):
    _, to, tc = R.KERNELS[kernel]
    for two in (False, True):
        A, B, dw0 = R.wgrad_operands(dims, two)
        assert float(dw0.abs().max()) + R.L_WGRAD <= R.L_EXACT + 1e-9 - 1 and len(A) == (2 if two else 1)
        for products in (6, 3):
            ref = R.live_reference("wgrad", A, B, products, L=R.L_WGRAD, what="%s, %d segments" % (dims, len(A)))
            assert torch.equal((ref + dw0).float().double(), ref + dw0)
            for a, b in zip(A, B):
                assert R.assert_wgrad_groups_live(a, b, products, to, tc) == products * (dims[0] * dims[1] * dims[2] // 64)
