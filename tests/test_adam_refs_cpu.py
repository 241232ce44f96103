"""Pins tests/adam_refs.py, the numpy restatements that tests/test_adam_ops_gpu.py compares the optimizer-step kernels with bit
for bit: the update against torch.optim.Adam in fp64 (yardstick: torch's own fp32 Adam on the same inputs), the bias corrections
against the formulae in 60-digit decimal arithmetic, the 16-bit roundings against torch's conversions, the slab sum's error and
-- the point of it -- that the ORDER of the sum is visible on the inputs the GPU tests use, and that the reference is finite on
the special inputs.  No GPU."""
import decimal

import numpy as np
import pytest
import torch

from adam_refs import (F32, HYPER, SLAB_NSPLITS, adam_hyper_ref, adam_table_ref, adam_upd_ref, normal_inputs, round_h16_ref,
                       slab_inputs, slab_inputs_h16, slab_lanes, slab_sum_ref, special_inputs, widen_h16_ref, wire_table_ref)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_update_against_torch_adam_in_fp64(wd):
    """20 steps on 1e5 elements.  The reference's largest error against torch.optim.Adam run in fp64 is at most twice that of
    torch's own fp32 Adam (single-tensor path) against the same fp64 run: the two fp32 computations differ in the grouping of
    sqrt(v) / sqrt(bc2) and of the moments' updates, not in accuracy."""
    n, steps = 100_000, 20
    lr, b1, b2, eps = HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"]
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 0.1 for _ in range(steps)]
    runs = {}
    for dt in (torch.float64, torch.float32):
        p = torch.nn.Parameter(p0.to(dt).clone())
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
        for g in grads:
            p.grad = g.to(dt).clone()
            opt.step()
        st = opt.state[p]
        runs[dt] = [t.detach().numpy().astype(np.float64) for t in (p, st["exp_avg"], st["exp_avg_sq"])]
    p, m, v = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, g in enumerate(grads, 1):
        p, m, v = adam_upd_ref(p, g.numpy(), m, v, adam_hyper_ref(t, lr, b1, b2, eps, wd))
    assert not np.array_equal(p, p0.numpy())
    same = float(np.mean(p == runs[torch.float32][0].astype(np.float32)))
    print("wd %g: %.1f %% of p bit-identical to torch fp32" % (wd, 100 * same))
    for name, mine, r64, r32 in zip("pmv", (p, m, v), runs[torch.float64], runs[torch.float32]):
        e_ref, e_t32 = float(np.abs(mine.astype(np.float64) - r64).max()), float(np.abs(r32 - r64).max())
        print("wd %g %s: reference vs fp64 %.3g, torch fp32 vs fp64 %.3g" % (wd, name, e_ref, e_t32))
        assert e_t32 > 0
        assert e_ref <= 2 * e_t32, "wd %g %s: reference vs fp64 %.3g, torch fp32 vs fp64 %.3g" % (wd, name, e_ref, e_t32)


@pytest.mark.parametrize("step", [1, 2, 10, 1000, 10 ** 5, 10 ** 6])
def test_hyper_against_decimal(step):
    """lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) in 60 significant digits on the exact values of the double arguments.  The double
    evaluation carries a relative error of a few 2^-53 (at step 2, 1 - b2^2 cancels to 2e-3: about 2^-44), which moves the fp32
    rounding only for an exact value within that distance of a tie: half an ulp times (1 + 2^-16)."""
    decimal.getcontext().prec = 60
    D = decimal.Decimal
    for lr, b1, b2, eps, wd, ginv in ((4e-4, 0.5, 0.999, 1e-8, 0.0, 1.0), (1e-3, 0.9, 0.999, 1e-8, 1e-2, 2.0 ** -12)):
        h = adam_hyper_ref(step, lr, b1, b2, eps, wd, ginv)
        assert h.dtype == np.float32 and h.shape == (12,)
        exact = {0: D(b1), 1: D(b2), 2: 1 - D(b1), 3: 1 - D(b2), 4: D(eps), 5: D(lr) / (1 - D(b1) ** step),
                 6: 1 / (1 - D(b2) ** step).sqrt(), 7: D(wd), 8: D(ginv)}
        for i, ex in exact.items():
            ulp = D(float(np.spacing(F32(float(ex)))))
            err = abs(D(float(h[i])) - ex)
            assert err <= ulp / 2 * (1 + D(2) ** -16), (step, i, float(h[i]), float(ex), float(err / ulp))
        assert h[9] == 0 and h[10] == 0 and h[11] == 0
        assert adam_hyper_ref(step, lr, b1, b2, eps, wd, ginv, skip=1)[9] == 1
        if step >= 16000:                                          # b2 = 0.999: 1 / sqrt(bc2) is within one fp32 ulp of 1
            assert abs(float(h[6]) - 1.0) <= 2.0 ** -23
    assert adam_hyper_ref(1, 4e-4, 0.5, 0.999, 1e-8)[5] == F32(8e-4)


def _rounding_points(half):
    """every finite value of the type, every tie between two neighbours and both fp32 neighbours of each tie; fp32 denormals;
    the overflow thresholds; infinities"""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    vals = widen_h16_ref(bits, half)
    vals = np.sort(vals[np.isfinite(vals)])
    with np.errstate(all="ignore"):
        ties = ((vals[:-1].astype(np.float64) + vals[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64), (vals[:-1].astype(np.float64) + vals[1:].astype(np.float64)) / 2)      # exact in fp32
    top = float(vals[-1])
    over = top + (top - float(vals[-2])) / 2                       # the tie between the largest finite value and "the next one"
    extra = np.array([1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 5.9604645e-8, 2.9802322e-8, 2.9802326e-8, 2.98023e-8,
                      np.inf, -np.inf, 65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 3.3895314e38, 3.4028235e38],
                     dtype=np.float32)
    if over < 3.4028235e38:
        o = F32(over)
        extra = np.concatenate([extra, [o, -o, np.nextafter(o, F32(0)), np.nextafter(o, F32(np.inf))]]).astype(np.float32)
    return np.concatenate([vals, ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)), extra])


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_rounding_against_torch(half):
    x = _rounding_points(half)
    dt = torch.bfloat16 if half == "bf16" else torch.float16
    want = torch.from_numpy(x).to(dt).view(torch.int16).numpy().view(np.uint16)
    got = round_h16_ref(x, half)
    assert got.dtype == np.uint16
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d of %d differ, first: x %r got %#x want %#x" % (bad.size, x.size, x[bad[0]], got[bad[0]], want[bad[0]])
    assert np.array_equal(widen_h16_ref(want, half).view(np.uint32), torch.from_numpy(want.view(np.int16)).view(dt).float().numpy().view(np.uint32))
    # the named cases, spelled out
    inf = 0x7F80 if half == "bf16" else 0x7C00
    assert round_h16_ref(np.array([np.inf, -np.inf], np.float32), half).tolist() == [inf, inf | 0x8000]
    if half == "f16":
        assert round_h16_ref(np.array([65504.0, 65519.996, 65520.0, 2.9802322e-8, 2.9802326e-8], np.float32), half).tolist() == \
            [0x7BFF, 0x7BFF, 0x7C00, 0x0000, 0x0001]             # overflow from the tie on; the tie at half the smallest denormal -> even
    else:
        assert round_h16_ref(np.array([1.00390625, 1.01171875, 3.39e38, 3.4e38], np.float32), half).tolist() == \
            [0x3F80, 0x3F82, 0x7F7F, 0x7F80]                     # ties to even; the largest finite value; overflow
    # NaN stays NaN with its sign (its payload is not specified: torch and the hardware may differ there)
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    r = round_h16_ref(nan, half)
    assert np.isnan(widen_h16_ref(r, half)).all() and ((r >> 15) == [0, 1, 0, 1]).all()
    assert torch.from_numpy(nan).to(dt).isnan().all()


@pytest.mark.parametrize("nsplit", SLAB_NSPLITS)
def test_slab_sum_error_and_order(nsplit):
    """(1) |slab_sum_ref - fp64 sum| <= nsplit 2^-24 sum|slab| per column.  (2) For nsplit > 4 (more than one lane) the kernel's
    order differs BITWISE from a plain sequential sum in at least a quarter of the columns of the fp32 inputs of the GPU tests
    (a condition on the inputs: with less, a kernel summing in another order could pass)."""
    n = 1028
    s = slab_inputs(nsplit, n)
    assert s.dtype == np.float32 and s.shape == (nsplit, n)
    k = np.log2(np.abs(s) + 1e-30)
    assert k.min() < -8 and k.max() > 5                            # the magnitudes are spread
    got = slab_sum_ref(s, nsplit)
    err = np.abs(got.astype(np.float64) - s.astype(np.float64).sum(0))
    bound = nsplit * 2.0 ** -24 * np.abs(s).astype(np.float64).sum(0)
    assert np.all(err <= bound), float((err / bound).max())
    seq = np.zeros(n, np.float32)
    for z in range(nsplit):
        seq = seq + s[z]
    share = float(np.mean(got.view(np.uint32) != seq.view(np.uint32)))
    h16 = {}
    for half in ("bf16", "f16"):
        w = widen_h16_ref(slab_inputs_h16(nsplit, n, half), half)
        sq = np.zeros(n, np.float32)
        for z in range(nsplit):
            sq = sq + w[z]
        h16[half] = float(np.mean(slab_sum_ref(w, nsplit).view(np.uint32) != sq.view(np.uint32)))
    print("nsplit %3d (%2d lanes): kernel order != sequential order in %.2f of the fp32 columns (bf16 slabs %.2f, fp16 slabs %.2f)"
          % (nsplit, slab_lanes(nsplit), share, h16["bf16"], h16["f16"]))
    if nsplit <= 4:
        assert share == 0.0                                        # one lane: the sequential sum
    else:
        assert share >= 0.25
        # ... and from the order with the lanes combined last to first (the other way round the LDS loop)
        SL = slab_lanes(nsplit)
        lanes = [slab_sum_ref(s[l::SL], len(range(l, nsplit, SL))) if len(range(l, nsplit, SL)) <= 4 else None for l in range(SL)]
        if all(x is not None for x in lanes):
            rev = lanes[0]
            for x in lanes[:0:-1]:
                rev = rev + x
            assert float(np.mean(got.view(np.uint32) != rev.view(np.uint32))) >= 0.1


def test_lane_boundaries():
    assert [slab_lanes(k) for k in (1, 4, 5, 32, 33, 200)] == [1, 1, 4, 4, 16, 16]
    # at 32 and 33 the result depends on the lane count: a kernel switching one slab early or late is seen
    for nsplit, other in ((32, 16), (33, 4), (5, 1)):
        s = slab_inputs(nsplit, 1028)
        parts = []
        for l in range(other):
            a = np.zeros(1028, np.float32)
            for z in range(l, nsplit, other):
                a = a + s[z]
            parts.append(a)
        alt = parts[0]
        for a in parts[1:]:
            alt = alt + a
        assert float(np.mean(slab_sum_ref(s, nsplit).view(np.uint32) != alt.view(np.uint32))) >= 0.25, nsplit


def test_tables():
    """adam_table_ref / wire_table_ref on plain | fp32 slabs | skipped | 16-bit slabs: each segment is the plain functions on its
    slice; a skipped segment keeps what it had."""
    half = "bf16"
    n = [8, 64, 12, 64, 7]
    off = np.concatenate([[0], np.cumsum(n)]).tolist()
    total = off[-1]
    p, g, m, v = normal_inputs(total, later=True)
    s32, s16 = slab_inputs(5, 64), slab_inputs_h16(33, 64, half)
    table = [(off[0], n[0], None, 0), (off[1], n[1], s32, 5), (off[2], n[2], None, -1), (off[3], n[3], s16, 33), (off[4], n[4], None, 0)]
    hyper = adam_hyper_ref(3, wd=1e-2, ginv=0.125, **HYPER)
    sh0 = np.full(total, 0x1234, np.uint16)
    P, M, V, S = adam_table_ref(p, g, m, v, hyper, table, half, shadow=sh0)
    W = wire_table_ref(g, table, half, wire=sh0)
    grads = [g[off[0]:off[1]], slab_sum_ref(s32, 5), None, slab_sum_ref(widen_h16_ref(s16, half), 33), g[off[4]:]]
    for i, gi in enumerate(grads):
        sl = slice(off[i], off[i + 1])
        if gi is None:
            assert np.array_equal(P[sl], p[sl]) and np.array_equal(M[sl], m[sl]) and np.array_equal(V[sl], v[sl])
            assert (S[sl] == 0x1234).all() and (W[sl] == 0x1234).all()
            continue
        pw, mw, vw = adam_upd_ref(p[sl], gi, m[sl], v[sl], hyper)
        assert np.array_equal(P[sl], pw) and np.array_equal(M[sl], mw) and np.array_equal(V[sl], vw)
        assert not np.array_equal(P[sl], p[sl])
        assert np.array_equal(S[sl], round_h16_ref(pw, half)) and np.array_equal(W[sl], round_h16_ref(gi, half))
    assert np.array_equal(p, normal_inputs(total, later=True)[0])              # inputs are not modified


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("ginv", [1.0, 0.125])
def test_reference_is_finite_on_the_special_inputs(wd, ginv):
    for step in (1, 7):
        p, g, m, v = special_inputs(64, wd)
        assert np.isfinite(g * F32(1 / ginv)).all()
        hyper = adam_hyper_ref(step, wd=wd, ginv=ginv, **HYPER)
        P, M, V = adam_upd_ref(p, g * F32(1 / ginv), m, v, hyper)
        for a in (P, M, V):
            assert np.isfinite(a).all()
        # the same through a 16-bit wire (bf16 as it is; fp16 with the large gradient clipped to 4096 so that 8 x it stays finite)
        for half, gw in (("bf16", g), ("f16", np.clip(g, -4096.0, 4096.0).astype(np.float32))):
            w = widen_h16_ref(round_h16_ref(gw * F32(1 / ginv), half), half)
            assert np.isfinite(w).all()
            for a in adam_upd_ref(p, w, m, v, hyper):
                assert np.isfinite(a).all()
        for half in ("bf16", "f16"):
            sh = widen_h16_ref(round_h16_ref(P, half), half)
            # the 16-bit shadow of a finite p: infinite only where p exceeds the type's range (fp16: the large entries)
            assert np.isfinite(sh[np.abs(P) < 60000]).all()
        # g = 0 with v = 0 and m = 0: denom = eps and p stays; a denormal g whose square underflows: v stays 0
        if wd == 0.0:
            assert P[0] == p[0] and V[0] == 0 and V[6] == 0 and M[6] != 0
        assert abs(P[10]) <= abs(p[10]) and abs(P[11]) <= abs(p[11])      # the large p steps towards zero (if the step is not absorbed)


def test_fp16_wire_overflow_case():
    """kept apart from the finite cases: a column whose fp32 sum exceeds 65504 goes onto an fp16 wire as infinity (bf16: finite)"""
    s = np.zeros((3, 8), np.float32)
    s[:, 2] = 30000.0
    s[:, 5] = -30000.0
    tot = slab_sum_ref(s, 3)
    assert tot[2] == 90000.0
    w = wire_table_ref(np.zeros(8, np.float32), [(0, 8, s, 3)], "f16")
    assert w.tolist() == [0, 0, 0x7C00, 0, 0, 0xFC00, 0, 0]
    assert np.isfinite(widen_h16_ref(wire_table_ref(np.zeros(8, np.float32), [(0, 8, s, 3)], "bf16"), "bf16")).all()
