"""(no GPU) tests/image_side_refs.py pinned against torch itself in fp64, every condition of part A of
tests/test_image_side_ops_gpu.py asserted on the very operands the GPU tests use (fixed seeds, drawn on the CPU), the dispatch
mirror checked against its own tables, and the tanh recipe of the last_up row kernels held inside its derived bound."""
import pytest
import torch
import torch.nn.functional as F

import image_side_refs as R

D = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("N,Ho,Wo,O", [(2, 3, 5, 4), (1, 1, 4, 6), (3, 2, 2, 2)])
def test_references_equal_torch_in_fp64(N, Ho, Wo, O):
    g = _gen(11)
    x = torch.randn(N, 3, 2 * Ho, 2 * Wo, generator=g, dtype=D)
    w = torch.randn(O, 3, 4, 4, generator=g, dtype=D)
    bd, bu = torch.randn(O, generator=g, dtype=D), torch.randn(3, generator=g, dtype=D)
    a = torch.randn(N, Ho, Wo, O, generator=g, dtype=D)
    ac = a.permute(0, 3, 1, 2)
    conv = F.conv2d(x, w, bd, stride=2, padding=1)
    assert torch.allclose(R.first_down(x, w, bd, 0.5), F.leaky_relu(conv, 0.5).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    assert torch.allclose(R.first_down(x, w), F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    m = R.signed_zeros((N, Ho, Wo, O), g).to(D)
    want = F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1) * torch.where(m > 0, 1.0, 0.5)
    assert torch.allclose(R.first_down(x, w, factor=R.mask_factor(m, 0.5)), want, rtol=0, atol=1e-12)
    assert torch.allclose(R.last_up(a, w, bu), F.conv_transpose2d(ac, w, bu, stride=2, padding=1), rtol=0, atol=1e-12)
    assert torch.allclose(R.last_up(a, w), F.conv_transpose2d(ac, w, stride=2, padding=1), rtol=0, atol=1e-12)
    dw = torch.nn.grad.conv2d_weight(x, (O, 3, 4, 4), ac, stride=2, padding=1)
    assert torch.allclose(R.wgrad(a, x), dw, rtol=0, atol=1e-12)
    # the fused input of rg_last_up_pre: train-mode batch norm with the batch's own statistics, then LeakyReLU
    mean, var = a.reshape(-1, O).mean(0), a.reshape(-1, O).var(0, unbiased=False)
    gamma, beta = torch.randn(O, generator=g, dtype=D), torch.randn(O, generator=g, dtype=D)
    want = F.leaky_relu(F.batch_norm(ac, None, None, gamma, beta, training=True, eps=1e-5), 0.5).permute(0, 2, 3, 1)
    assert torch.allclose(R.bn_act(a, mean, (var + 1e-5).rsqrt(), gamma, beta, 0.5), want, rtol=0, atol=1e-10)


def test_weight_gradient_is_the_gradient_of_first_down_and_last_up_its_adjoint():
    g = _gen(12)
    x = torch.randn(2, 3, 6, 8, generator=g, dtype=D)
    w = torch.randn(5, 3, 4, 4, generator=g, dtype=D, requires_grad=True)
    a = torch.randn(2, 3, 4, 5, generator=g, dtype=D)
    (R.first_down(x, w) * a).sum().backward()
    assert torch.allclose(w.grad, R.wgrad(a, x), rtol=0, atol=1e-12)
    wd = w.detach()
    assert abs(float((R.first_down(x, wd) * a).sum() - (R.last_up(a, wd) * x).sum())) < 1e-10


def test_sign_words_and_post_rows():
    y = torch.zeros(3, 64)
    y[0, 0], y[0, 63], y[1, 5], y[2, 7] = 1.0, 2.0, -1.0, -0.0
    assert R.sign_words(y).tolist() == [1 - 2 ** 63, 0, 0]
    assert not R.words_hold_both_values(R.sign_words(y))
    g = _gen(13)
    assert R.words_hold_both_values(R.sign_words(R.signed_zeros((64, 64), g)))
    for name in ("row64", "seam3", "strips2", "strips565"):
        c = R.BY_NAME[name]
        v = torch.randn(c.N, 3, 2 * c.Ho, 2 * c.Wo, generator=g, dtype=D)
        rows = R.post_rows(c, v)                                  # the strips tile the output: the rows sum to the whole
        assert rows.shape == (R.post_blocks(c), 4) and torch.allclose(rows.sum(0), R.post_sums(v), rtol=1e-12, atol=1e-9)


def test_head_references_equal_torch_in_fp64():
    g = _gen(14)
    N, C = 5, 7
    a = torch.randn(N, 16, C, generator=g, dtype=D)
    w = torch.randn(C, 16, generator=g, dtype=D, requires_grad=True)
    gh = torch.randn(N, generator=g, dtype=D)
    # the head is Conv2d(C, 1, 4, 1, 0) on a 4 x 4 map: a[n][tap][c] is the NHWC activation, w[c][tap] the OIHW weight
    conv = F.conv2d(a.view(N, 4, 4, C).permute(0, 3, 1, 2), w.view(1, C, 4, 4)).view(N)
    h, out = R.head_fwd(a, w, 3.0, 0.5)
    assert torch.allclose(h, conv + 3.0, rtol=0, atol=1e-12) and torch.allclose(out, F.leaky_relu(conv + 3.0, 0.5), rtol=0, atol=1e-12)
    ar = a.clone().requires_grad_(True)
    (R.head_fwd(ar, w, None, 1.0)[0] * gh).sum().backward()
    assert torch.allclose(ar.grad.reshape(N, -1), R.head_bwd_data(gh, w.detach()), rtol=0, atol=1e-12)
    assert torch.allclose(w.grad, R.head_wgrad(gh, a), rtol=0, atol=1e-12)
    hv = torch.tensor([-2.0, -0.0, 0.0, 3.0], dtype=D, requires_grad=True)
    F.leaky_relu(hv, 0.5).sum().backward()
    assert torch.equal(R.head_grad(hv.detach(), 1.0, 0.5), hv.grad)           # torch, too, gives the slope at zero


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_part_a_conditions_hold_on_the_committed_seeds(c):
    p = R.operands(c)
    R.operand_ranges(c, p)
    if c.name in R.LARGE:
        return                                                    # ranges and S bounds alone (the device test asserts the rest)
    if "d" in c.ops:
        R.down_refs(c, p)
    if "u" in c.ops:
        R.up_refs(c, p)
    if "w" in c.ops:
        R.wgrad_refs(c, p)


def test_case_tables_reach_every_kernel_and_path():
    seen = {"d": set(), "u": set(), "w": set()}
    for c in R.CASES:
        for opts in R.variants(c):
            for op, fn in (("d", R.kernel_first_down), ("u", R.kernel_last_up), ("w", R.kernel_wgrad)):
                if op in c.ops:
                    seen[op].add(fn(c, opts))
    assert seen["d"] == {"first_down_rows_kernel", "first_down_rows128_kernel", "first_down_kernel<h16>", "first_down_kernel<float>",
                         "rg_generic_first_down"}
    assert seen["u"] == {"last_up_rows_kernel", "last_up_rows128_kernel", "last_up_kernel<h16, 8>", "last_up_kernel<float, 4, 16>",
                         "rg_generic_last_up"}
    assert seen["w"] == {"skinny_wgrad_rows_kernel", "skinny_wgrad_rows128_kernel", "skinny_wgrad_kernel<h16>",
                         "skinny_wgrad_kernel<float>", "rg_generic_skinny_wgrad"}
    B = R.BY_NAME
    assert {R.chunk_of(B[n].Wo) for n in ("row32_h2", "row64", "row128")} == {32, 64, 128}
    assert [B[n].Wo // R.chunk_of(B[n].Wo) for n in ("seam2", "seam3")] == [2, 3]
    assert [R.strip_of(B[n].Ho) for n in ("strips2", "strips10", "strips1", "strips12", "strips565")] == [16, 10, 1, 12, 1]
    assert R.units(B["units775"]) == 775 > R.SK_ROWS_BLOCKS and -(-775 // 768) == 2 and 775 - 387 * 2 == 1     # 387 blocks of 2, one of 1
    assert R.strips(B["strips565"]) == 565 > R.LU_BLOCKS
    assert R.units(B["r128_n1"]) == 128 and R.strips(B["r128_n1"]) == 8 and R.units(B["r128_n7"]) == 896
    assert R.units(B["r128_n5"]) == 640 and R.wgrad_slabs(B["r128_n5"], {"skinny128": 1}) == 512
    assert R.wgrad_slabs(B["r128_n5"], {"skinny128": 0}) == 640 and R.wgrad_slabs(B["r128_n7"], {"skinny128": 0}) == 768
    assert B["row32_h2"].Ho == 1 and not R.wgrad_live(B["row32_h2"])[:, 0].any() and R.wgrad_live(B["row64"]).all()
    # both sides of rg_generic_f32_image_side
    assert R.f32_generic(B["f32_o64"], 1) and not R.f32_generic(B["f32_o64"], 0) and not R.f32_generic(B["f32_o64_np2"], 1)


def test_head_operands():
    for N in R.HEAD_N + [257]:
        h = R.head_h_values(N)
        assert bool((h == 0).any()) and bool(torch.signbit(h[h == 0]).any())
        if N > 2:
            assert bool((h > 0).any()) and bool((h < 0).any())
        for C in R.HEAD_C:
            if N == 257:
                continue
            a, w, gh = R.head_operands(N, C)
            assert R.in_set(a, [-2.0, -1.0, 1.0, 2.0]) and R.in_set(w, [-1.0, 0.0, 1.0]) and torch.equal(4 * gh, (4 * gh).round())
            assert 2 * 16 * C + 3 <= 2 ** 24 and 2 * 2 * N * 0.75 <= 2 ** 24          # S of h, and of dw accumulated once
            assert bool((gh != 0).any()) and float(gh.abs().max()) <= 0.75       # gh * w is a 16-bit number
            hh, _ = R.head_fwd(a, w, R.HEAD_BIAS, 0.5)
            assert N < 7 or hh.unique().numel() > 1
            assert bool((R.head_wgrad(gh, a) != 0).any())


def test_bound_units():
    assert R.UNIT[torch.bfloat16] == 2.0 ** -8 and R.UNIT[torch.float16] == 2.0 ** -11 and R.UNIT[torch.float32] == 0.0
    for dt, u in R.UNIT.items():                                   # the largest relative rounding error of the type is u / (1 + u) < u
        if u:
            v = torch.tensor(1.0 + u, dtype=D)
            assert float(v.to(dt)) in (1.0, 1.0 + 2 * u)
    ref, S = torch.tensor([2.0], dtype=D), torch.tensor([8.0], dtype=D)
    assert float(R.bound(ref, S, 48, 2.0 ** -8)) == 2.0 ** -8 * 2 + 48 * 2.0 ** -24 * (1 + 2.0 ** -8) * 8 + 2.0 ** -25


def test_tanh_recipe_stays_inside_its_derived_bound():
    """x = k 2^-10 over [-20, 20]; every step of the recipe pushed by its unit in both directions (32 patterns)"""
    x = torch.arange(-20 * 1024, 20 * 1024 + 1, dtype=D) / 1024
    ref = torch.tanh(x)
    worst = 0.0
    for signs in R.tanh_sign_patterns():
        worst = max(worst, float((R.tanh_recipe(x, signs) - ref).abs().max()))
    print("tanh recipe: worst emulated |err| = %.3e, bound %.3e" % (worst, R.TANH_RECIPE_BOUND))
    assert worst <= R.TANH_RECIPE_BOUND
    assert worst >= 0.25 * R.TANH_RECIPE_BOUND, "the bound is not loose by more than the sign patterns explain"
    # the sup used in the derivation: |2 y e^y / (e^y + 1)^2| <= 0.4478
    y = torch.arange(0, 40 * 1024, dtype=D) / 1024
    assert float((2 * y * torch.exp(y) / (torch.exp(y) + 1) ** 2).max()) <= 0.4478
    # the recipe itself in fp32 (the CPU's correctly rounded exp2 and division are within the 1 ulp the units are given)
    x32 = x.float()
    got = 1 - 2 / (torch.exp2(x32 * torch.tensor(R.TANH_C, dtype=torch.float32)) + 1)
    assert float((got.double() - torch.tanh(x32.double())).abs().max()) <= R.TANH_RECIPE_BOUND
    assert float(R.TANH_BIAS[0]) * 64 == -21 and torch.equal(R.TANH_BIAS * 64, (R.TANH_BIAS * 64).round())
