"""The references and conditions of tests/test_bn_reduce_ops_gpu.py, without a kernel.

* every expression tree of tests/bn_reduce_refs.py against torch autograd in fp64: BatchNorm + LeakyReLU forward and backward,
  the tangent through torch.func.jvp, the double backward through autograd.grad(create_graph=True), and against
  oracle.ops_ref.RefOps(torch.float64);
* every exactness and non-triviality condition of parts A, C and D on the operands the GPU file uses;
* the mirror of make_plan: every value of every plan field occurs, with both element sizes;
* the two-phase rank simulation against RefOps with a real stat_reduce (a sum over simulated ranks) and the whole batch.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_reduce_refs as B
import vae_fid_refs as R
from oracle.ops_ref import RefOps

EPS = 1e-5
H16 = [torch.bfloat16, torch.float16, torch.float32]


def _close(a, b, what, tol=1e-10):
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= tol, "%s: %.3e" % (what, err)


def _fp64_case(M, C, seed):
    """fp64 operands with z's own batch statistics as mean / invstd (what autograd differentiates through)"""
    z, ga, zt, qa = (R.gauss((M, C), seed + i) for i in range(4))
    z = z * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * R.gauss((C,), seed + 4), 0.1 * R.gauss((C,), seed + 5)
    mean = z.mean(0)
    invstd = torch.rsqrt(((z - mean) ** 2).mean(0) + EPS)
    return {"z": z, "ga": ga, "zt": zt, "qa": qa, "mean": mean, "invstd": invstd, "gamma": gamma, "beta": beta, "slope": 0.2}


def _bn_lrelu(z, gamma, beta, slope):
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return F.leaky_relu((z - mean) * torch.rsqrt(var + EPS) * gamma + beta, slope)


@pytest.mark.parametrize("M,C", [(37, 6), (64, 12), (300, 37)])
def test_trees_against_autograd_fp64(M, C):
    o = _fp64_case(M, C, 900 + M)
    fam = B.Family(o, False, strict_leaves=False)
    slope = fam.p.slope
    z = o["z"].clone().requires_grad_(True)
    gamma, beta = o["gamma"].clone().requires_grad_(True), o["beta"].clone().requires_grad_(True)
    a = _bn_lrelu(z, gamma, beta, slope)
    _close(fam.a.v, a.detach(), "forward")
    assert torch.equal(F.batch_norm(o["z"], None, None, o["gamma"], o["beta"], True, 0.1, EPS).gt(0), fam.y.v.gt(0))
    # backward: gz, dgamma = s_gyxh, dbeta = s_gy
    gz, dg, db = torch.autograd.grad(a, (z, gamma, beta), o["ga"], create_graph=True)
    _close(fam.gz.v, gz.detach(), "gz")
    _close(fam.s_gyxh.v, dg.detach(), "dgamma = s_gyxh")
    _close(fam.s_gy.v, db.detach(), "dbeta = s_gy")
    # tangent: jvp of the whole forward in direction zt
    _, at = torch.func.jvp(lambda t: _bn_lrelu(t, o["gamma"], o["beta"], slope), (o["z"],), (o["zt"],))
    _close(fam.at.v, at, "tangent")
    _close(fam.s_zt.v, o["zt"].sum(0), "s_zt")
    # double backward: <ga1, at> = <gz, zt>, so pz = d/dz [<qa, a> + <gz(z), zt>], dgamma / dbeta likewise
    for use_qa in (True, False):
        L = (gz * o["zt"]).sum() + ((a * o["qa"]).sum() if use_qa else 0.0)
        pz, dg2, db2 = torch.autograd.grad(L, (z, gamma, beta), retain_graph=True, allow_unused=True)
        d = fam.dbl[use_qa]
        _close(d["pz"].v, pz, "pz qa=%s" % use_qa, 1e-9)
        _close(d["dg"].v, dg2, "double backward dgamma qa=%s" % use_qa, 1e-9)
        if use_qa:
            _close(d["db"].v, db2, "double backward dbeta")
        else:
            assert not bool(d["db"].v.any()) and (db2 is None or float(db2.abs().max()) < 1e-12)
    # every bound is finite and small next to the values it gates
    for ev in (fam.a, fam.gz, fam.at, fam.dbl[True]["pz"], fam.s_gy, fam.s_xhzt):
        assert torch.isfinite(ev.e).all() and float(ev.e.max()) < 1e-3 * float(ev.v.abs().max())


@pytest.mark.parametrize("M,C", [(37, 6), (64, 12)])
def test_trees_against_refops_fp64(M, C):
    o = _fp64_case(M, C, 950 + M)
    fam = B.Family(o, False, strict_leaves=False)
    ref = RefOps(torch.float64)
    sl = fam.p.slope                                  # the fp32 number the kernels receive
    n = lambda t: t.reshape(1, M, 1, C)
    v = [o[k] for k in ("mean", "invstd", "gamma", "beta")]
    _close(fam.a.v, ref.bn_act(n(o["z"]), *v, sl).reshape(M, C), "bn_act")
    dg, db = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    gz, s_gy, s_gyxh = ref.bn_act_bwd(n(o["z"]), n(o["ga"]), *v, sl, dg, db, False)
    _close(fam.gz.v, gz.reshape(M, C), "gz")
    at, s_zt, s_xhzt = ref.bn_tangent(n(o["z"]), n(o["zt"]), *v, sl)
    _close(fam.at.v, at.reshape(M, C), "at")
    for use_qa in (True, False):
        pz = ref.bn_double_bwd(n(o["z"]), n(o["qa"]) if use_qa else None, n(o["zt"]), n(o["ga"]), *v, sl, s_gy, s_gyxh, s_zt, s_xhzt,
                               dg, db, False)
        _close(fam.dbl[use_qa]["pz"].v, pz.reshape(M, C), "pz", 1e-9)
        _close(fam.dbl[use_qa]["dg"].v, dg, "dgamma", 1e-9)
        assert float((fam.dbl[use_qa]["db"].v - db).abs().max()) < 1e-10
    s, ss = ref.bn_stats(n(o["z"]))
    _close(fam.sum_z.v, s, "sum"), _close(fam.sum_zz.v, ss, "sumsq")
    out = torch.zeros(C, dtype=torch.float64)
    ref.col_sum(n(o["ga"]), out, False)
    _close(fam.colsum_ga.v, out, "col_sum")


def test_statistics_reference_against_torch_batchnorm():
    M, C = 300, 12
    z = R.gauss((M, C), 77) * 2 + 3
    rm0, rv0 = 0.1 * R.gauss((C,), 78), 1 + 0.1 * R.gauss((C,), 79).abs()
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
    bn(z)
    r = B.stats_ref(z, M, EPS, 0.1, rm0, rv0)
    _close(r["rm"], bn.running_mean, "running_mean"), _close(r["rv"], bn.running_var, "running_var")
    _close(r["mean"], z.mean(0), "mean"), _close(r["invstd"], torch.rsqrt(z.var(0, unbiased=False) + EPS), "invstd", 1e-9)
    assert int(bn.num_batches_tracked) == 1
    for k in ("e_mean", "e_invstd", "e_rm", "e_rv"):
        assert torch.isfinite(r[k]).all() and bool((r[k] > 0).all())


@pytest.mark.parametrize("ratio,gated", [(0, True), (8, True), (64, False)])       # (at 257 rows; at 1031 rows 8 is beyond it too)
def test_statistics_offset_mean_where_the_bound_applies(ratio, gated):
    """the GPU file's statement -- the summation bound on the variance stays below one 16-bit rounding unit of invstd at |mean| /
    std = 0 and 8 and not at 64 -- is a property of the reference alone"""
    z64 = (R.gauss((257, 37), 400 + ratio) + float(ratio)).float().double()
    r = B.stats_ref(z64, 257, float(np.float32(EPS)), float(np.float32(0.1)), None, None)
    assert bool((r["e_invstd"] <= B.UNIT[torch.bfloat16] * r["invstd"]).all()) == gated


def test_latent_reference_against_torch():
    u, z = 0.17 * R.gauss((7, 50), 35), R.gauss((7, 50), 36)
    for split in (False, True):
        ref, bnd = B.latent_ref(u, z, split)
        n = u + z
        _close(ref, (n - n.mean(0)) / n.std(0), "latent_prep")
        assert torch.isfinite(bnd).all() and float(bnd.max()) < 1e-4


# ------------------------------------------------------------------ make_plan
def test_make_plan_mirror_covers_every_plan_field():
    for esize in (2, 4):
        plans = {mc: B.make_plan(mc[0], mc[1], esize) for mc in B.PLAN_CASES}
        assert {p["vec"] for p in plans.values()} == ({8, 4, 1} if esize == 2 else {4, 1})
        assert {p["tx"] for p in plans.values()} == {8, 16, 32}
        assert {1, 2} <= {p["gx"] for p in plans.values()}
        # gx = 2 with a partly empty second column block
        assert any(p["gx"] == 2 and mc[1] < 2 * p["tx"] * p["vec"] for mc, p in plans.items())
        # two rounds of the finisher's 32 lanes with a 7-row last block; one block; a ragged last block
        assert any(p["gy"] == 33 and p["last"] == 7 for p in plans.values())
        assert any(p["gy"] == 1 for p in plans.values()) and any(1 < p["gy"] <= 32 for p in plans.values())
        # rows per thread = ceil((rpb - ty) / TY) <= 4 by construction (gy = ceil(M / 4 TY)): the U-remainder loop alone (no
        # thread has four rows), the unrolled body alone (every thread has four), and blocks where some threads take the body and
        # the others the remainder (with U = 2, the double backward, three rows are one body trip and one remainder row)
        assert any(p["rpb"] <= 3 * p["ty"] for p in plans.values()) and any(p["rpb"] == 4 * p["ty"] for p in plans.values())
        assert any(3 * p["ty"] < p["rpb"] < 4 * p["ty"] for p in plans.values())
    p = B.make_plan(1031, 37, 2)
    assert (p["vec"], p["tx"], p["gx"], p["gy"], p["rpb"], p["last"]) == (1, 32, 2, 33, 32, 7)
    p = B.make_plan(1024, 136, 2)
    assert (p["vec"], p["tx"], p["gx"]) == (8, 16, 2)
    assert B.make_plan(64, 68, 4)["tx"] == 16
    # the single-launch form's smallest shapes: C / vec == 32
    assert 256 // 8 == 32 and 128 // 4 == 32
    assert len(set(B.plan_id(M, C, 2) for M, C in B.PLAN_CASES)) == len(B.PLAN_CASES)


# ------------------------------------------------------------------ part A: conditions
ALL_EXACT = B.PLAN_CASES + B.FUSED_CASES[2] + B.FUSED_CASES[4]


@pytest.mark.parametrize("M,C", ALL_EXACT)
def test_exact_conditions_hold(M, C):
    """every node of every tree is an fp32 number (asserted inside Family), every stored operand and the forward's result
    survive the storage types, and the non-triviality conditions hold -- at the level of exactness exact_level(M) states"""
    ops = B.exact_operands(M, C, B.EXACT_SEED.get((M, C), 1))
    pow2, pz = B.exact_level(M)
    fam = B.Family(ops, True, applies=pow2, dbl_apply=pz)
    for dtype in H16:
        B.exact_conditions(ops, fam, dtype, "%dx%d" % (M, C), pow2)
    assert float(ops["slope"]) == 0.5 and set(torch.unique(ops["invstd"]).tolist()) <= {0.5, 1.0}
    assert set(torch.unique(ops["gamma"].abs()).tolist()) <= {1.0, 2.0, 4.0}
    assert torch.equal(ops["beta"] * 2, torch.round(ops["beta"] * 2)) and torch.equal(ops["mean"], torch.round(ops["mean"]))
    # what exact_level leaves to the bound really is inexact there, or the level would be too modest
    fb = B.Family(ops, False, y_exact=True)
    assert torch.isfinite(fb.dbl[True]["pz"].e).all()
    if pow2 and not pz:
        with pytest.raises(AssertionError):
            B.Family(ops, True)
    # the mask convention: y == 0 takes slope
    y0 = fam.y.v == 0
    assert int(y0.sum()) >= 1 and bool((fam.mk.v[y0] == 0.5).all()) and bool((fam.a.v[y0] == 0).all())


@pytest.mark.parametrize("C", [8, 37, 136])
def test_rank_case_exact_conditions_hold(C):
    """part C, W = 2 with 32 rows per rank: the whole batch of 64 rows is exact down to pz, and so is each rank's share"""
    M = 64
    ops = B.exact_operands(M, C, B.EXACT_SEED.get((M, C), 1))
    fam = B.Family(ops, True)
    for dtype in H16:
        B.exact_conditions(ops, fam, dtype, "W2 32x%d" % C, True)
    tot = {q: torch.zeros(C, dtype=torch.float64) for q in (True, False)}
    for k in range(2):
        fk = B.Family(ops, True, rows=B.rank_rows(32, 2, k))
        for q in (True, False):
            tot[q] += fk.dbl[q]["dg"].v
            assert torch.equal(fk.dbl[q]["pz"].v, fam.dbl[q]["pz"].v)
        assert not torch.equal(fk.dbl[True]["dg"].v, fam.dbl[True]["dg"].v)          # a share, not the whole
    for q in (True, False):
        assert torch.equal(tot[q], fam.dbl[q]["dg"].v)


# ------------------------------------------------------------------ part C: the two-phase simulation on the torch twin
@pytest.mark.parametrize("W,Mr,C", [(2, 32, 8), (3, 32, 37), (3, 343, 8)])
def test_two_phase_simulation_equals_whole_batch(W, Mr, C):
    M = W * Mr
    o = B.gauss_operands(M, C, 100, torch.float32)
    whole, sim = RefOps(torch.float64), RefOps(torch.float64)
    sl = float(np.float32(0.2))
    n = lambda t: t.reshape(1, t.shape[0], 1, C)
    part = lambda key, k: n(o[key][B.rank_rows(Mr, W, k)])
    v = [o[k] for k in ("mean", "invstd", "gamma", "beta")]
    z64 = torch.zeros(C, dtype=torch.float64)
    # --- backward
    dgW, dbW = z64.clone(), z64.clone()
    gzW, sgyW, sgxW = whole.bn_act_bwd(n(o["z"]), n(o["ga"]), *v, sl, dgW, dbW, False)
    dgs, dbs = [z64.clone() for _ in range(W)], [z64.clone() for _ in range(W)]
    outs = B.two_phase(sim, W, lambda k: sim.bn_act_bwd(part("z", k), part("ga", k), *v, sl, dgs[k], dbs[k], False))
    _close(torch.cat([x[0] for x in outs], 1), gzW, "gz")
    _close(outs[0][1], sgyW, "s_gy"), _close(sum(dgs), dgW, "dgamma over the ranks"), _close(sum(dbs), dbW, "dbeta over the ranks")
    # --- a REAL stat_reduce (all ranks at once) gives the same as the two phases: the local sums do not depend on the total
    loc = [RefOps(torch.float64) for _ in range(W)]
    got = []
    for k in range(W):
        others = [(part("z", j), part("ga", j)) for j in range(W) if j != k]

        def real_reduce(t, k=k, others=others, calls={"i": 0}):
            # rank k's tensor plus what every other rank computes for the same call
            idx = calls["i"]
            calls["i"] += 1
            for zj, gj in others:
                r = RefOps(torch.float64)
                t.add_(r.bn_act_bwd(zj, gj, *v, sl)[1 + idx])
        loc[k].stat_reduce, loc[k].stat_world = real_reduce, W
        got.append(loc[k].bn_act_bwd(part("z", k), part("ga", k), *v, sl)[0])
    _close(torch.cat(got, 1), torch.cat([x[0] for x in outs], 1), "two phases against a real reduction", 1e-12)
    # --- tangent, double backward with and without qa, accumulate both ways
    atW, sztW, sxzW = whole.bn_tangent(n(o["z"]), n(o["zt"]), *v, sl)
    tan = B.two_phase(sim, W, lambda k: sim.bn_tangent(part("z", k), part("zt", k), *v, sl))
    _close(torch.cat([x[0] for x in tan], 1), atW, "at")
    fam = B.Family(o, False)
    for use_qa in (True, False):
        for accumulate in (False, True):
            start = R.ints((C,), 5, -7, 7)
            dgW, dbW = start.clone(), start.clone()
            pzW = whole.bn_double_bwd(n(o["z"]), n(o["qa"]) if use_qa else None, n(o["zt"]), n(o["ga"]), *v, sl, sgyW, sgxW, sztW,
                                      sxzW, dgW, dbW, accumulate)
            dgs, dbs = [start.clone() for _ in range(W)], [start.clone() for _ in range(W)]
            first = {"on": True}

            def dbl(k):
                if not first["on"]:
                    dgs[k].copy_(start), dbs[k].copy_(start)
                return sim.bn_double_bwd(part("z", k), part("qa", k) if use_qa else None, part("zt", k), part("ga", k), *v, sl,
                                         outs[0][1], outs[0][2], tan[0][1], tan[0][2], dgs[k], dbs[k], accumulate)
            pzs = B.two_phase(sim, W, dbl, first)
            _close(torch.cat(pzs, 1), pzW, "pz", 1e-9)
            a0 = start if accumulate else 0.0
            _close(sum(dgs) - W * a0, dgW - a0, "double backward dgamma over the ranks", 1e-9)
            assert float((sum(dbs) - W * a0 - (dbW - a0)).abs().max()) < 1e-9
            # the trees' rank shares are RefOps' rank shares
            for k in range(W):
                fk = B.Family(o, False, rows=B.rank_rows(Mr, W, k))
                _close(fk.dbl[use_qa]["dg"].v, dgs[k] - a0, "rank share of dgamma", 1e-9)
            _close(fam.dbl[use_qa]["pz"].v, pzW.reshape(M, C), "tree pz", 1e-9)
    # --- forward (split branch), latent_prep, the squared norm
    rmW, rvW, nbW = z64.clone(), z64.clone() + 1, torch.zeros((), dtype=torch.int64)
    aW, meanW, invW = whole.bn_forward(n(o["z"]), o["gamma"], o["beta"], sl, EPS, 0.1, rmW, rvW, nbW)
    rms, rvs, nbs = [z64.clone() for _ in range(W)], [z64.clone() + 1 for _ in range(W)], [torch.zeros((), dtype=torch.int64) for _ in range(W)]
    first = {"on": True}

    def fwd(k):
        if not first["on"]:
            rms[k].zero_(), rvs[k].fill_(1.0), nbs[k].zero_()
        return sim.bn_forward(part("z", k), o["gamma"], o["beta"], sl, EPS, 0.1, rms[k], rvs[k], nbs[k])
    f = B.two_phase(sim, W, fwd, first)
    _close(torch.cat([x[0] for x in f], 1), aW, "a"), _close(f[1][1], meanW, "mean"), _close(f[1][2], invW, "invstd")
    _close(rms[1], rmW, "running_mean"), _close(rvs[1], rvW, "running_var")
    assert int(nbs[0]) == 1
    u, zz = 0.17 * R.gauss((M, 50), 1), R.gauss((M, 50), 2)
    lp = B.two_phase(sim, W, lambda k: sim.latent_prep(u[B.rank_rows(Mr, W, k)], zz[B.rank_rows(Mr, W, k)]))
    _close(torch.cat(lp), whole.latent_prep(u, zz), "latent_prep", 1e-9)
    _close(torch.cat(lp), B.latent_ref(u, zz, True)[0], "latent_ref", 1e-9)
    x = R.gauss((W, 1027), 3)
    sq = B.two_phase(sim, W, lambda k: sim.stat_allreduce(sim.sqnorm(x[k])))
    _close(sq[0], (x * x).sum().reshape(1), "sqnorm over the ranks")


# ------------------------------------------------------------------ part D: partial rows
def _group_row(r, grp, groups, Gb):
    """rg_bn.hip group_row"""
    return ((r // Gb) * groups + grp) * Gb + r % Gb


@pytest.mark.parametrize("G", [1, 31, 33, 512, 513, 1000, 2052])
@pytest.mark.parametrize("C", [8, 136, 36])
def test_partial_rows_conditions_hold(G, C):
    M = 4096
    z = B.ints_z(M, C, 600 + G + C)
    part = B.partial_rows(z, G)
    B.partial_condition(part, z, M)
    assert part.shape == (G, 2, C)
    if G == 513:
        per = -(-G // 32)
        assert per == 17 and G - 30 * per == 3 and G - 31 * per < 0          # slice 30 is short, slice 31 empty
    # the two-group layouts: half h's row r sits at group_row(r, h, 2, G / nblk)
    z2 = torch.cat([B.ints_z(M, C, 700 + G + C), B.ints_z(M, C, 701 + G + C, -2, 4) * 2.0])
    for nblk in (1, 4):
        if G % nblk:
            continue
        p2 = B.partial_rows_g2(z2, G, nblk)
        for h in range(2):
            ph = B.partial_rows(z2[h * M:(h + 1) * M], G)
            B.partial_condition(ph, z2[h * M:(h + 1) * M], M)
            idx = torch.tensor([_group_row(r, h, 2, G // nblk) for r in range(G)])
            assert torch.equal(p2[idx], ph)
        if nblk == 4 and G >= 8:
            # dropping the "% Gb" term of group_row would read other rows: the layouts differ
            wrong = torch.tensor([min(((r // (G // 4)) * 2 + 0) * (G // 4), 2 * G - 1) for r in range(G)])
            assert not torch.equal(p2[wrong], B.partial_rows(z2[:M], G))
    assert not torch.equal(z2[:M].sum(0), z2[M:].sum(0))


def test_misc_exact_operands_are_exact():
    """the (A) halves of the rg_misc cases: every node an fp32 number"""
    n = 1027
    ctx = B.Ctx(True)
    L = ctx.leaf
    gy, y = R.ints((n,), 1, -4, 4), R.ints((n,), 2, -4, 4) * 0.25
    ctx.mul(L(gy), ctx.sub(L(1.0), ctx.mul(L(y), L(y))))
    real, fake = R.ints((n,), 3, -8, 8), R.ints((n,), 4, -8, 8)
    ctx.add(ctx.mul(L(0.25), L(real)), ctx.mul(ctx.sub(L(1.0), L(0.25)), L(fake)))
    x = R.ints((1024 * 256 + 5,), 11, -3, 3)
    s = ctx.colsum(B.EV((x * x)[:, None]))
    assert float(s.v) < 2 ** 24
    assert ctx.nodes >= 6
