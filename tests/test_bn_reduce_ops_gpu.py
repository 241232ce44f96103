"""The row-loop kernels of rg_bn.hip and the reductions / element-wise kernels of rg_misc.hip, op by op, through the C ABI.

Kinds of check (the pattern of tests/test_vae_fid_ops_gpu.py; references, operand builders and the expression trees are in
tests/bn_reduce_refs.py, pinned against torch autograd on the CPU by tests/test_bn_reduce_refs_cpu.py):
(A) EXACT.  Small integers in z / ga / zt / qa, integer mean, invstd, |gamma| and the slope powers of two, beta a multiple of
    1/2: every node of a kernel's expression tree is an fp32 number (asserted on the reference before comparing), so every sum
    must be torch.equal to the fp64 one at every plan of make_plan, and -- where 1 / M is exact -- every stored element must
    equal the fp64 value rounded once to the storage type.  y == 0 is planted in every case: the mask there is `slope`.
(B) BOUND.  Gaussian operands, slope 0.2: element-wise |got - ref| <= the bound the SAME tree gives when every node adds one
    rounding unit of its own magnitude to the propagated error of its inputs, a column sum the any-order term (M - 1) 2^-24
    sum |t_i| and the store one unit of the storage type.  Nothing in a bound is measured; every worst |err| / bound is printed
    as "RATIO <op> <case> <value>" (profiles/bn_reduce_op_errors.txt records them).
(C) RANKS.  Synchronised statistics on W simulated ranks of one GPU: every op runs on every part with a stat_reduce that records
    the part's local tensor, then again with a stat_reduce that writes the recorded total; stat_world = W both times.
(D) PARTIAL ROWS.  Hand-built integer column sums [G][2][C] through the finishers, narrow and two-level.
(S) SENTINEL, in every test: outputs inside a pattern-filled allocation, operands and per-channel vectors inside NaN-filled ones,
    the workspace exactly what the query / HipOps asks for inside a guarded allocation, every guard intact after every call, one
    byte less of workspace refused with RG_EWORKSPACE before any launch.
"""
import numpy as np
import pytest
import torch

import bn_reduce_refs as B
import vae_fid_refs as R
from both_builds import fp16_twin
from guarded import DEV, SBITS, Guarded
from vae_fid_refs import SENTINEL, U32, bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT16 = -24704.0                                   # a finite pattern bf16 and fp16 both hold (0xc6c1 / 0xf608)
RG_EWORKSPACE = -3
EPS, MOM = float(np.float32(1e-5)), float(np.float32(0.1))      # what the kernels receive (floats)


class _Env:
    def __init__(self, dtype):
        from rna_gan_amd import _abi
        from rna_gan_amd.ops_hip import HipOps
        self.abi = _abi
        self.ops = HipOps(dtype, DEV)
        self.lib = self.ops.lib
        self.dtype = dtype
        self.dt = self.ops.dt

    @property
    def stream(self):
        return self.ops.stream

    def ok(self, rc, what):
        self.abi.check(rc, what)
        torch.cuda.synchronize()


def _name(dtype):
    return {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]


def _ptr(t):
    return 0 if t is None else (t.t if isinstance(t, Guarded) else t).data_ptr()


def _ibits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def _pattern(dtype, value):
    return int(_ibits(torch.full((1,), value, dtype=dtype)).item())


def _keeps(g, value):
    """the surroundings of a Guarded of any element size keep the fill bit for bit (element-wise views: an odd offset is fine)"""
    pat = _pattern(g.flat.dtype, value)
    head, tail = g.flat[:g.before].clone(), g.flat[g.before + g.n:].clone()
    return bool((_ibits(head) == pat).all()) and bool((_ibits(tail) == pat).all())


def _untouched(g, value):
    return bool((_ibits(g.t.clone()) == _pattern(g.flat.dtype, value)).all())


class Bufs:
    """every buffer of a test, with what must surround it; check() after every call"""

    def __init__(self):
        self.ins, self.outs = [], []

    def operand(self, t64, dtype, rows_after=0):
        """an operand in its storage type inside NaN: `after` covers 4 x 32 rows past the last one and a 16-byte load past C"""
        C = t64.shape[-1] if t64.dim() else 1
        g = Guarded(t64.float().to(dtype), NAN, after=(128 * C + 64 + rows_after) // 64 * 64 + 64)
        self.ins.append(g)
        return g

    def vec(self, t64):
        g = Guarded(t64.float(), NAN, after=1024)
        self.ins.append(g)
        return g

    def out(self, shape, dtype=torch.float32, init=None):
        """init = None: pattern-filled (the op writes all of it); a tensor: the values an accumulating op adds to"""
        fill = SENTINEL if dtype == torch.float32 else SENT16
        body = torch.full(shape, fill, dtype=dtype) if init is None else init.float().to(dtype)
        g = Guarded(body, fill, after=(128 * (shape[-1] if len(shape) else 1) + 128) // 64 * 64)
        g.fill = fill
        self.outs.append(g)
        return g

    def ws(self, nbytes):
        assert nbytes % 4 == 0
        g = Guarded(torch.full((nbytes // 4,), SENTINEL, dtype=torch.float32), SENTINEL, after=8192)
        g.fill, g.nbytes = SENTINEL, nbytes
        self.outs.append(g)
        return g

    def check(self, what):
        for g in self.outs:
            assert _keeps(g, g.fill), what + ": wrote outside an output or the workspace"
        for g in self.ins:
            body = g.t.clone().float()
            assert torch.isfinite(body).all(), what + ": an operand was overwritten"


def _cpu(g):
    return (g.t if isinstance(g, Guarded) else g).detach().cpu()


def _equal(got, ref64, dtype, what):
    """(A): the stored result equals the fp64 value rounded once to the storage type (by value: -0.0 == +0.0)"""
    got = _cpu(got)
    assert torch.isfinite(got.float()).all(), what + ": non-finite output (a guard region was read?)"
    want = ref64.float().to(dtype).reshape(got.shape)
    bad = got != want
    assert not bool(bad.any()), "%s: %d of %d outputs differ, first at %s: got %s want %s" % (
        what, int(bad.sum()), bad.numel(), bad.nonzero()[:3].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


def _within(got, x, dtype, op, case, extra=None):
    """(B): |got - ref| <= the tree's bound; the worst ratio is printed"""
    got = _cpu(got).double()
    ref, bnd = B.store_bound(x, dtype)
    ref, bnd = ref.reshape(got.shape), bnd.reshape(got.shape)
    if extra is not None:
        bnd = bnd + extra
    assert torch.isfinite(got).all(), "%s %s: non-finite output (a guard region was read?)" % (op, case)
    err = (got - ref).abs()
    ratio = float((err / bnd).max())
    print("RATIO %s %s %.4f" % (op, case, ratio))
    bad = err > bnd
    assert not bool(bad.any()), "%s %s: %d of %d outputs outside the bound (worst ratio %.2f), first at %s" % (
        op, case, int(bad.sum()), bad.numel(), ratio, bad.nonzero()[:4].tolist())


def _chk(got, ev_exact, ev_bound, dtype, op, case):
    if ev_exact is not None:
        _equal(got, ev_exact.v, dtype, "%s[%s]" % (op, case))
    else:
        _within(got, ev_bound, dtype, op, case)


def _refused(env, rc, outs, what):
    """one byte less of workspace: RG_EWORKSPACE and nothing launched (every output still holds its pattern)"""
    torch.cuda.synchronize()
    assert rc == RG_EWORKSPACE, "%s with one byte less of workspace returned %d" % (what, rc)
    for g in outs:
        assert _untouched(g, g.fill), what + ": launched although it refused the workspace"


# ================================================================== the BatchNorm family on one operand set
def _run_family(env, ops, fam_x, fam_b, case, refuse=True):
    """Every op of the family through the C ABI on the operands `ops`.  fam_x: Family in exact mode (what it lacks -- see
    bn_reduce_refs.exact_level -- is held to fam_b, the same trees in bound mode) or None (part B: everything to fam_b)."""
    lib, dtype, dt, st = env.lib, env.dtype, env.dt, env.stream
    M, C = ops["z"].shape
    slope = float(ops["slope"])
    X = lambda name: None if fam_x is None or not hasattr(fam_x, name) else getattr(fam_x, name)
    XD = lambda qa, name: None if fam_x is None or name not in fam_x.dbl[qa] else fam_x.dbl[qa][name]
    b = Bufs()
    z, ga, zt, qa = (b.operand(ops[k], dtype) for k in ("z", "ga", "zt", "qa"))
    mean, invstd, gamma, beta = (b.vec(ops[k]) for k in ("mean", "invstd", "gamma", "beta"))
    q2, q3 = lib.rg_colreduce_workspace_bytes(M, C, 2), lib.rg_colreduce_workspace_bytes(M, C, 3)
    q1 = lib.rg_colreduce_workspace_bytes(M, C, 1)
    ws1, ws2, ws3 = b.ws(q1), b.ws(q2), b.ws(q3)
    # ---- bn_stats
    s, ss = b.out((C,)), b.out((C,))
    if refuse:
        _refused(env, lib.rg_bn_stats(_ptr(z), _ptr(s), _ptr(ss), M, C, dt, _ptr(ws2), q2 - 1, st), [s, ss, ws2], "rg_bn_stats")
    env.ok(lib.rg_bn_stats(_ptr(z), _ptr(s), _ptr(ss), M, C, dt, _ptr(ws2), q2, st), "rg_bn_stats")
    _chk(s, X("sum_z"), fam_b.sum_z, torch.float32, "bn_stats.sum", case)
    _chk(ss, X("sum_zz"), fam_b.sum_zz, torch.float32, "bn_stats.sumsq", case)
    b.check("bn_stats")
    # ---- col_sum: written, then accumulated onto integers
    acc0 = R.ints((C,), 5, -7, 7)
    o1, o2 = b.out((C,)), b.out((C,), init=acc0)
    if refuse:
        _refused(env, lib.rg_col_sum(_ptr(ga), _ptr(o1), M, C, dt, 0, _ptr(ws1), q1 - 1, st), [o1, ws1], "rg_col_sum")
    env.ok(lib.rg_col_sum(_ptr(ga), _ptr(o1), M, C, dt, 0, _ptr(ws1), q1, st), "rg_col_sum")
    env.ok(lib.rg_col_sum(_ptr(ga), _ptr(o2), M, C, dt, 1, _ptr(ws1), q1, st), "rg_col_sum")
    _chk(o1, X("colsum_ga"), fam_b.colsum_ga, torch.float32, "col_sum", case)
    cx = None if X("colsum_ga") is None else B.EV(X("colsum_ga").v + acc0)
    cb = B.EV(fam_b.colsum_ga.v + acc0, fam_b.colsum_ga.e)             # (+ one rounding of the sum: the store's unit)
    _chk(o2, cx, cb, torch.float32, "col_sum.acc", case)
    b.check("col_sum")
    # ---- bn_act
    a = b.out((M, C), dtype)
    env.ok(lib.rg_bn_act(_ptr(z), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(a), M, C, slope, dt, st), "rg_bn_act")
    _chk(a, X("a"), fam_b.a, dtype, "bn_act", case)
    b.check("bn_act")
    # ---- bn_act_bwd: dgamma / dbeta written, then accumulated; then both halves of a double batch at once
    for accumulate in (0, 1):
        gz, s_gy, s_gyxh = b.out((M, C), dtype), b.out((C,)), b.out((C,))
        dg, db = (b.out((C,), init=acc0), b.out((C,), init=-acc0)) if accumulate else (b.out((C,)), b.out((C,)))
        args = lambda nbytes: (_ptr(z), _ptr(ga), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(gz), _ptr(s_gy),
                               _ptr(s_gyxh), _ptr(dg), _ptr(db), accumulate, M, C, slope, dt, _ptr(ws2), nbytes, st)
        if refuse and not accumulate:
            _refused(env, lib.rg_bn_act_bwd(*args(q2 - 1)), [gz, s_gy, s_gyxh, dg, db], "rg_bn_act_bwd")
        env.ok(lib.rg_bn_act_bwd(*args(q2)), "rg_bn_act_bwd")
        sfx = ".acc" if accumulate else ""
        _chk(s_gy, X("s_gy"), fam_b.s_gy, torch.float32, "bn_act_bwd.s_gy", case)
        _chk(s_gyxh, X("s_gyxh"), fam_b.s_gyxh, torch.float32, "bn_act_bwd.s_gyxh", case)
        a0 = acc0 if accumulate else 0.0
        _chk(dg, None if fam_x is None else B.EV(fam_x.s_gyxh.v + a0), B.EV(fam_b.s_gyxh.v + a0, fam_b.s_gyxh.e),
             torch.float32, "bn_act_bwd.dgamma" + sfx, case)
        _chk(db, None if fam_x is None else B.EV(fam_x.s_gy.v - a0), B.EV(fam_b.s_gy.v - a0, fam_b.s_gy.e),
             torch.float32, "bn_act_bwd.dbeta" + sfx, case)
        _chk(gz, X("gz"), fam_b.gz, dtype, "bn_act_bwd.gz", case)
        b.check("bn_act_bwd")
    _run_bwd2(env, ops, fam_x, fam_b, case, acc0)
    # ---- bn_tangent
    at, s_zt, s_xhzt = b.out((M, C), dtype), b.out((C,)), b.out((C,))
    targs = lambda nbytes: (_ptr(z), _ptr(zt), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(at), _ptr(s_zt),
                            _ptr(s_xhzt), M, C, slope, dt, _ptr(ws2), nbytes, st)
    if refuse:
        _refused(env, lib.rg_bn_tangent(*targs(q2 - 1)), [at, s_zt, s_xhzt], "rg_bn_tangent")
    env.ok(lib.rg_bn_tangent(*targs(q2)), "rg_bn_tangent")
    _chk(s_zt, X("s_zt"), fam_b.s_zt, torch.float32, "bn_tangent.s_zt", case)
    _chk(s_xhzt, X("s_xhzt"), fam_b.s_xhzt, torch.float32, "bn_tangent.s_xhzt", case)
    _chk(at, X("at"), fam_b.at, dtype, "bn_tangent.at", case)
    b.check("bn_tangent")
    # ---- bn_double_bwd, with and without qa, written and accumulated; its sums come from the kernels above (inside the bound of
    # the fp64 sums, which is what the tree's leaves carry; equal to them in exact mode)
    sv = [b.vec(_cpu(t).double()) for t in (s_gy, s_gyxh, s_zt, s_xhzt)]
    for use_qa in (True, False):
        for accumulate in (0, 1):
            pz = b.out((M, C), dtype)
            dg, db = (b.out((C,), init=acc0), b.out((C,), init=-acc0)) if accumulate else (b.out((C,)), b.out((C,)))
            dargs = lambda nbytes: (_ptr(z), _ptr(qa) if use_qa else 0, _ptr(zt), _ptr(ga), _ptr(mean), _ptr(invstd), _ptr(gamma),
                                    _ptr(beta), _ptr(sv[0]), _ptr(sv[1]), _ptr(sv[2]), _ptr(sv[3]), _ptr(pz), _ptr(dg), _ptr(db),
                                    accumulate, M, C, slope, dt, _ptr(ws3), nbytes, st)
            if refuse and use_qa and not accumulate:
                _refused(env, lib.rg_bn_double_bwd(*dargs(q3 - 1)), [pz, dg, db, ws3], "rg_bn_double_bwd")
            env.ok(lib.rg_bn_double_bwd(*dargs(q3)), "rg_bn_double_bwd")
            tag = "%s%s" % ("+qa" if use_qa else "", ".acc" if accumulate else "")
            a0 = acc0 if accumulate else 0.0
            xdg, xdb = XD(use_qa, "dg"), XD(use_qa, "db")
            bdg, bdb = fam_b.dbl[use_qa]["dg"], fam_b.dbl[use_qa]["db"]
            _chk(dg, None if xdg is None else B.EV(xdg.v + a0), B.EV(bdg.v + a0, bdg.e), torch.float32, "bn_double_bwd.dgamma" + tag, case)
            _chk(db, None if xdb is None else B.EV(xdb.v - a0), B.EV(bdb.v - a0, bdb.e), torch.float32, "bn_double_bwd.dbeta" + tag, case)
            _chk(pz, XD(use_qa, "pz"), fam_b.dbl[use_qa]["pz"], dtype, "bn_double_bwd.pz" + tag, case)
            b.check("bn_double_bwd")
    # ---- lrelu_bwd on (ga, a): the mask from the sign of the stored activation, a == 0 (planted) takes `slope`
    ctx = B.Ctx(fam_x is not None)
    a64 = _cpu(a).double()
    if fam_x is not None:
        assert int((a64 == 0).sum()) >= 1
    lr = ctx.mul(ctx.leaf(ops["ga"]), B.EV(torch.where(a64 > 0, torch.ones_like(a64), torch.full_like(a64, fam_b.p.slope))), "lrelu_bwd")
    ag = b.operand(a64, dtype)
    out = b.out((M, C), dtype)
    env.ok(lib.rg_lrelu_bwd(_ptr(ga), _ptr(ag), _ptr(out), M * C, slope, dt, st), "rg_lrelu_bwd")
    _chk(out, lr if fam_x is not None else None, lr, dtype, "lrelu_bwd", case)
    b.check("lrelu_bwd")


def _run_bwd2(env, ops, fam_x, fam_b, case, acc0):
    """rg_bn_act_bwd_g2 on a double batch whose halves are (ops, ops with ga negated): gz per half, s_gy / s_gyxh [2][C], dgamma
    / dbeta = the sum over both halves = 0 exactly when written, the start values when accumulated.  The workspace is twice
    rg_colreduce_workspace_bytes(M, C, 2), as HipOps.bn_act_bwd2 passes."""
    lib, dtype, dt, st = env.lib, env.dtype, env.dt, env.stream
    M, C = ops["z"].shape
    b = Bufs()
    z2 = b.operand(torch.cat([ops["z"], ops["z"]]), dtype)
    ga2 = b.operand(torch.cat([ops["ga"], -ops["ga"]]), dtype)
    mean, invstd = (b.vec(torch.stack([ops[k], ops[k]])) for k in ("mean", "invstd"))
    gamma, beta = b.vec(ops["gamma"]), b.vec(ops["beta"])
    q = 2 * lib.rg_colreduce_workspace_bytes(M, C, 2)
    ws = b.ws(q)
    for accumulate in (0, 1):
        gz, s_gy, s_gyxh = b.out((2 * M, C), dtype), b.out((2, C)), b.out((2, C))
        dg, db = (b.out((C,), init=acc0), b.out((C,), init=-acc0)) if accumulate else (b.out((C,)), b.out((C,)))
        args = lambda nbytes: (_ptr(z2), _ptr(ga2), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), _ptr(gz), _ptr(s_gy),
                               _ptr(s_gyxh), _ptr(dg), _ptr(db), accumulate, M, C, float(ops["slope"]), dt, _ptr(ws), nbytes, st)
        if not accumulate:
            _refused(env, lib.rg_bn_act_bwd_g2(*args(q - 1)), [gz, s_gy, s_gyxh, dg, db, ws], "rg_bn_act_bwd_g2")
        env.ok(lib.rg_bn_act_bwd_g2(*args(q)), "rg_bn_act_bwd_g2")
        neg = lambda ev: B.EV(-ev.v, ev.e)
        both = lambda ev: B.EV(torch.stack([ev.v, -ev.v]), torch.stack([ev.e, ev.e]))
        cat = lambda ev: B.EV(torch.cat([ev.v, -ev.v]), torch.cat([ev.e, ev.e]))
        x = fam_x
        _chk(s_gy, None if x is None else both(x.s_gy), both(fam_b.s_gy), torch.float32, "bn_act_bwd2.s_gy", case)
        _chk(s_gyxh, None if x is None else both(x.s_gyxh), both(fam_b.s_gyxh), torch.float32, "bn_act_bwd2.s_gyxh", case)
        _chk(gz, None if x is None or not hasattr(x, "gz") else cat(x.gz), cat(fam_b.gz), dtype, "bn_act_bwd2.gz", case)
        a0 = acc0 if accumulate else torch.zeros_like(acc0)
        # the two halves' sums cancel: a0 + s - s'.  In bound mode each half's sum carries its own error.
        _chk(dg, None if x is None else B.EV(a0.clone()), B.EV(a0.clone(), 2 * fam_b.s_gyxh.e + 2 * U32 * fam_b.s_gyxh.v.abs()),
             torch.float32, "bn_act_bwd2.dgamma" + (".acc" if accumulate else ""), case)
        _chk(db, None if x is None else B.EV(-a0), B.EV(-a0, 2 * fam_b.s_gy.e + 2 * U32 * fam_b.s_gy.v.abs()), torch.float32,
             "bn_act_bwd2.dbeta" + (".acc" if accumulate else ""), case)
        b.check("bn_act_bwd_g2")


def _families(ops, M, dtype, what):
    pow2, pz = B.exact_level(M)
    fam_x = B.Family(ops, True, applies=pow2, dbl_apply=pz)
    B.exact_conditions(ops, fam_x, dtype, what, pow2)
    fam_b = B.Family(ops, False, y_exact=True)
    return fam_x, fam_b


def _plan_ids(esize):
    return [B.plan_id(M, C, esize) for M, C in B.PLAN_CASES]


def _exact_case(M, C, dtype, case):
    env = _Env(dtype)
    ops = B.exact_operands(M, C, B.EXACT_SEED.get((M, C), 1))
    fam_x, fam_b = _families(ops, M, dtype, case)
    _run_family(env, ops, fam_x, fam_b, case)


@fp16_twin
@pytest.mark.parametrize("M,C", B.PLAN_CASES, ids=_plan_ids(2))
def test_family_exact_every_plan(M, C, h16=torch.bfloat16):
    """(A) + (S) at every plan of make_plan, 16-bit storage, both builds (the id names the reduction's plan)."""
    _exact_case(M, C, h16, "%s/%s" % (_name(h16), B.plan_id(M, C, 2)))


@pytest.mark.parametrize("M,C", B.PLAN_CASES, ids=_plan_ids(4))
def test_family_exact_every_plan_f32(M, C):
    """(A) + (S) at every plan of make_plan, fp32 storage (vec = 4 at most: other plans for the same shapes)."""
    _exact_case(M, C, torch.float32, "f32/" + B.plan_id(M, C, 4))


@fp16_twin
@pytest.mark.parametrize("M", [64, 300])
def test_family_exact_single_launch(M, monkeypatch, h16=torch.bfloat16):
    """(A) + (S) on the single-launch form (RNAGAN_BN_FUSED=1) at its smallest 16-bit shapes: C / vec = 32, M = 64 (its
    threshold) and 300 (a second, ragged trip of the 256-thread row loop)."""
    monkeypatch.setenv("RNAGAN_BN_FUSED", "1")
    assert (M, 256) in B.FUSED_CASES[2]
    _exact_case(M, 256, h16, "%s/fused-M%dxC256" % (_name(h16), M))


@pytest.mark.parametrize("M", [64, 300])
def test_family_exact_single_launch_f32(M, monkeypatch):
    monkeypatch.setenv("RNAGAN_BN_FUSED", "1")
    assert (M, 128) in B.FUSED_CASES[4]
    _exact_case(M, 128, torch.float32, "f32/fused-M%dxC128" % M)


BOUND_CASES = [(1, 37), (37, 6), (64, 12), (64, 68), (1031, 37), (1024, 136), (1031, 264)]


def _bound_case(M, C, dtype):
    env = _Env(dtype)
    ops = B.gauss_operands(M, C, 100, dtype)
    fam_b = B.Family(ops, False)
    _run_family(env, ops, None, fam_b, "%s/%s" % (_name(dtype), B.plan_id(M, C, 4 if dtype == torch.float32 else 2)), refuse=False)


@fp16_twin
@pytest.mark.parametrize("M,C", BOUND_CASES)
def test_family_bound_gaussian(M, C, h16=torch.bfloat16):
    """(B) + (S): Gaussian operands, slope 0.2, arbitrary gamma / beta, M <= 1031; 16-bit storage, both builds."""
    _bound_case(M, C, h16)


@pytest.mark.parametrize("M,C", BOUND_CASES)
def test_family_bound_gaussian_f32(M, C):
    _bound_case(M, C, torch.float32)


LRELU_N = [1, 7, 8, 9, 8 * 256 * 8192 + 8]


@fp16_twin
@pytest.mark.parametrize("n", LRELU_N)
def test_lrelu_bwd_sizes(n, h16=torch.bfloat16):
    """out = g * (a > 0 ? 1 : slope) bit for bit (slope 1/2, integer g: one exact product), a == 0 planted; n = 1, 7, 9 take
    the scalar kernel, 8 one vector, 8 * 256 * 8192 + 8 one whole grid sweep of the vector kernel plus one vector (16-bit) /
    two sweeps (fp32)."""
    for dtype in (h16, torch.float32) if h16 == torch.bfloat16 else (h16,):
        env = _Env(dtype)
        gen = torch.Generator().manual_seed(n % 1000)
        g = torch.randint(-3, 4, (n,), generator=gen).to(dtype)
        a = torch.randint(-3, 4, (n,), generator=gen).to(dtype)
        a[::5] = 0
        want = (g.float() * torch.where(a.float() > 0, 1.0, 0.5)).to(dtype)
        assert n < 16 or 0.2 <= float((a.float() > 0).float().mean()) <= 0.8
        gg, ag = Guarded(g, NAN, after=4096), Guarded(a, NAN, after=4096)
        out = Guarded(torch.full((n,), SENTINEL if dtype == torch.float32 else SENT16, dtype=dtype),
                      SENTINEL if dtype == torch.float32 else SENT16, after=4096)
        env.ok(env.lib.rg_lrelu_bwd(_ptr(gg), _ptr(ag), _ptr(out), n, 0.5, env.dt, env.stream), "rg_lrelu_bwd")
        assert torch.equal(out.t, want.to(DEV)), "lrelu_bwd n=%d %s" % (n, _name(dtype))
        assert _keeps(out, SENTINEL if dtype == torch.float32 else SENT16), "lrelu_bwd wrote outside its output"


# ================================================================== statistics
def _stat_bufs(b, C, seed):
    rm0, rv0 = (0.1 * R.gauss((C,), seed)).float().double(), (1 + 0.1 * R.gauss((C,), seed + 1).abs()).float().double()
    rm, rv = b.out((C,), init=rm0), b.out((C,), init=rv0)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    return rm0, rv0, rm, rv, nbt


def _check_stats(case, op, r, mean, invstd, rm, rv, gate_var=True):
    ev = lambda v, e: B.EV(v, e)
    _within(mean, ev(r["mean"], r["e_mean"] - U32 * r["mean"].abs()), torch.float32, op + ".mean", case)
    if gate_var:
        _within(invstd, ev(r["invstd"], r["e_invstd"]), torch.float32, op + ".invstd", case)
    if rm is not None:
        _within(rm, ev(r["rm"], r["e_rm"]), torch.float32, op + ".running_mean", case)
        if gate_var:
            _within(rv, ev(r["rv"], r["e_rv"]), torch.float32, op + ".running_var", case)


STAT_CASES = [(64, 12), (1024, 37), (1024, 136), (1031, 264), (37, 6)]


@fp16_twin
@pytest.mark.parametrize("M,C", STAT_CASES)
def test_statistics_three_calls(M, C, h16=torch.bfloat16):
    _statistics_three_calls(M, C, h16)


@pytest.mark.parametrize("M,C", STAT_CASES)
def test_statistics_three_calls_f32(M, C):
    _statistics_three_calls(M, C, torch.float32)


def _statistics_three_calls(M, C, dtype):
    """bn_stats_finalize, bn_forward and bn_stats + bn_finalize in a row on integer z: with M a power of two mean is BIT-EQUAL
    (the column sum is exact, the quotient a dyadic rational); invstd and the running statistics within the counted roundings of
    StatsFinalizeFin (bn_reduce_refs.stats_ref); num_batches_tracked == 3 after the three calls; bn_forward's activation equals
    bn_act's on the mean / invstd it wrote (the same functor on the same fp32 parameters: bit for bit)."""
    env = _Env(dtype)
    lib, dt, st = env.lib, env.dt, env.stream
    case = "%s/%dx%d" % (_name(dtype), M, C)
    z64 = B.ints_z(M, C, 300 + C)
    b = Bufs()
    z = b.operand(z64, dtype)
    gamma, beta = b.vec(R.pow2_affine(C, 3)[0]), b.vec(R.pow2_affine(C, 3)[1] * 0.5)
    rm0, rv0, rm, rv, nbt = _stat_bufs(b, C, 310)
    q = lib.rg_colreduce_workspace_bytes(M, C, 2)
    ws = b.ws(q)
    pow2 = M & (M - 1) == 0
    zero = torch.zeros(C, dtype=torch.float64)
    E0 = (zero, zero)                                                  # integer z: both column sums are exact in fp32
    assert float((z64 * z64).sum(0).max()) < 2 ** 24
    r = B.stats_ref(z64, M, EPS, MOM, rm0, rv0, *E0)
    # 1: statistics + finalize in one pass
    mean, invstd = b.out((C,)), b.out((C,))
    _refused(env, lib.rg_bn_stats_finalize(_ptr(z), M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv), _ptr(nbt), dt,
                                           _ptr(ws), q - 1, st), [mean, invstd, ws], "rg_bn_stats_finalize")
    assert int(nbt.cpu()) == 0
    env.ok(lib.rg_bn_stats_finalize(_ptr(z), M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv), _ptr(nbt), dt,
                                    _ptr(ws), q, st), "rg_bn_stats_finalize")
    if pow2:
        _equal(mean, r["mean"], torch.float32, "bn_stats_finalize.mean[%s]" % case)
    _check_stats(case, "bn_stats_finalize", r, mean, invstd, rm, rv)
    assert int(nbt.cpu()) == 1
    b.check("bn_stats_finalize")
    # 2: the whole forward
    r2 = B.stats_ref(z64, M, EPS, MOM, r["rm"], r["rv"], *E0)
    r2["e_rm"], r2["e_rv"] = r2["e_rm"] + (1 - MOM) * r["e_rm"], r2["e_rv"] + (1 - MOM) * r["e_rv"]
    mean2, invstd2, a = b.out((C,)), b.out((C,)), b.out((M, C), dtype)
    fargs = lambda nbytes: (_ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean2), _ptr(invstd2), _ptr(rm), _ptr(rv),
                            _ptr(nbt), _ptr(a), dt, _ptr(ws), nbytes, st)
    _refused(env, lib.rg_bn_forward(*fargs(q - 1)), [mean2, invstd2, a], "rg_bn_forward")
    env.ok(lib.rg_bn_forward(*fargs(q)), "rg_bn_forward")
    assert torch.equal(bits(mean2.t), bits(mean.t)) and torch.equal(bits(invstd2.t), bits(invstd.t)), "bn_forward: other statistics"
    _check_stats(case, "bn_forward", r2, mean2, invstd2, rm, rv)
    a_act = b.out((M, C), dtype)
    env.ok(lib.rg_bn_act(_ptr(z), _ptr(mean2), _ptr(invstd2), _ptr(gamma), _ptr(beta), _ptr(a_act), M, C, 0.5, dt, st), "rg_bn_act")
    assert torch.equal(_ibits(a.t.clone()), _ibits(a_act.t.clone())), "bn_forward's activation is not bn_act's"
    assert int(nbt.cpu()) == 2
    b.check("bn_forward")
    # 3: bn_stats + bn_finalize
    r3 = B.stats_ref(z64, M, EPS, MOM, r2["rm"], r2["rv"], *E0)
    r3["e_rm"], r3["e_rv"] = r3["e_rm"] + (1 - MOM) * r2["e_rm"], r3["e_rv"] + (1 - MOM) * r2["e_rv"]
    s, ss, mean3, invstd3 = b.out((C,)), b.out((C,)), b.out((C,)), b.out((C,))
    env.ok(lib.rg_bn_stats(_ptr(z), _ptr(s), _ptr(ss), M, C, dt, _ptr(ws), q, st), "rg_bn_stats")
    _equal(s, z64.sum(0), torch.float32, "bn_stats.sum"), _equal(ss, (z64 * z64).sum(0), torch.float32, "bn_stats.sumsq")
    sv, ssv = b.vec(_cpu(s).double()), b.vec(_cpu(ss).double())
    env.ok(lib.rg_bn_finalize(_ptr(sv), _ptr(ssv), M, C, EPS, MOM, _ptr(mean3), _ptr(invstd3), _ptr(rm), _ptr(rv), _ptr(nbt), st),
           "rg_bn_finalize")
    assert torch.equal(bits(mean3.t), bits(mean.t)) and torch.equal(bits(invstd3.t), bits(invstd.t)), "bn_finalize: other statistics"
    _check_stats(case, "bn_finalize", r3, mean3, invstd3, rm, rv)
    assert int(nbt.cpu()) == 3
    b.check("bn_finalize")


@pytest.mark.parametrize("ratio", [0, 8, 64])
def test_statistics_offset_mean(ratio):
    """Gaussian z with |mean| / std = 0, 8, 64 (fp32 storage: the offset survives the store): the one-pass E[x^2] - E[x]^2 on
    fp32 sums loses accuracy as the ratio grows.  Where the summation bound on the variance, carried to invstd, is below one
    16-bit rounding unit of invstd, invstd is GATED at the counted bound; beyond that the measured error is only recorded
    (RECORD lines; profiles/bn_reduce_op_errors.txt)."""
    env = _Env(torch.float32)
    lib, st = env.lib, env.stream
    M, C = 257, 37                                     # (at 1031 rows the summation bound passes the 16-bit unit at ratio 8 already)
    z64 = (R.gauss((M, C), 400 + ratio) + float(ratio)).float().double()
    b = Bufs()
    z = b.operand(z64, torch.float32)
    rm0, rv0, rm, rv, nbt = _stat_bufs(b, C, 410)
    q = lib.rg_colreduce_workspace_bytes(M, C, 2)
    ws = b.ws(q)
    mean, invstd = b.out((C,)), b.out((C,))
    env.ok(lib.rg_bn_stats_finalize(_ptr(z), M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv), _ptr(nbt), env.dt,
                                    _ptr(ws), q, st), "rg_bn_stats_finalize")
    r = B.stats_ref(z64, M, EPS, MOM, rm0, rv0)
    applies = bool((r["e_invstd"] <= B.UNIT[torch.bfloat16] * r["invstd"]).all())
    got = _cpu(invstd).double()
    rel = float(((got - r["invstd"]).abs() / r["invstd"]).max())
    print("RECORD invstd ratio=%d gated=%d worst_rel_err=%.3e bound_rel=%.3e" % (
        ratio, int(applies), rel, float((r["e_invstd"] / r["invstd"]).max())))
    _check_stats("f32/ratio%d" % ratio, "bn_stats_finalize", r, mean, invstd, rm, rv, gate_var=applies)
    assert applies == (ratio < 64), "where the bound applies is a property of the reference: 0 and 8 gated, 64 recorded"
    b.check("bn_stats_finalize")


# ================================================================== (C) synchronised statistics on simulated ranks
def _two_phase(ops_obj, W, fn, first=None, bufs=None, what=""):
    """bn_reduce_refs.two_phase; every guard of `bufs` is checked after each phase"""
    def after(phase):
        torch.cuda.synchronize()
        if bufs is not None:
            bufs.check("%s %s" % (what, phase))
    return B.two_phase(ops_obj, W, fn, first, after)


@fp16_twin
@pytest.mark.parametrize("C", [8, 37, 136])
@pytest.mark.parametrize("W,Mr", [(2, 32), (3, 32), (2, 343), (3, 343)])
def test_sync_statistics_simulated_ranks(W, Mr, C, h16=torch.bfloat16):
    """(C): W = 2 with 32 rows per rank gets the exact operands of (A) and torch.equal, everything else the bound of (B);
    reference = the whole batch without synchronisation.  The concatenated outputs equal the whole-batch outputs, the per-rank
    dgamma / dbeta (written and accumulated) sum over the ranks to the whole-batch gradients.  (S): every rank's part of every
    operand is an allocation of its own inside NaN (the rows behind a rank's last row are NOT the next rank's), the per-channel
    vectors too; the in/out gradient buffers and the running statistics sit inside pattern-filled allocations; all guards are
    checked after each phase."""
    M = W * Mr
    exact = W == 2 and Mr == 32
    for dtype in (h16, torch.float32) if h16 == torch.bfloat16 else (h16,):
        env = _Env(dtype)
        hip = env.ops
        case = "%s/W%d-%dx%d" % (_name(dtype), W, Mr, C)
        if exact:
            ops = B.exact_operands(M, C, B.EXACT_SEED.get((M, C), 1))
            fam_x = B.Family(ops, True)
            B.exact_conditions(ops, fam_x, dtype, case, True)
            fam_b = fam_x
        else:
            ops = B.gauss_operands(M, C, 100, dtype)
            fam_x, fam_b = None, B.Family(ops, False)
        fks = [B.Family(ops, exact, rows=B.rank_rows(Mr, W, k)) for k in range(W)]
        slope = float(ops["slope"])
        b = Bufs()
        parts = {key: [b.operand(ops[key][B.rank_rows(Mr, W, k)], dtype) for k in range(W)] for key in ("z", "ga", "zt", "qa")}
        part = lambda key, k: parts[key][k].t
        vec = {k: b.vec(ops[k]).t for k in ("mean", "invstd", "gamma", "beta")}
        X = lambda name: None if fam_x is None else getattr(fam_x, name)
        acc0 = R.ints((C,), 5, -7, 7)
        f32 = lambda t: t.float().to(DEV)

        def grad_bufs(accumulate):
            """W pairs (dgamma, dbeta) inside pattern-filled allocations: start values +-acc0 when accumulating"""
            return ([b.out((C,), init=acc0 if accumulate else None) for _ in range(W)],
                    [b.out((C,), init=-acc0 if accumulate else None) for _ in range(W)])

        def rank_sum(gs):
            return torch.stack([_cpu(g).double() for g in gs]).sum(0)

        def acc_extra(local):
            """accumulate: rank k's buffer is fl32(acc0 + local_k): one rounding of the result per rank, on top of the sums' own"""
            return sum(U32 * (acc0.abs() + l.v.abs() + l.e) for l in local)
        # ---- bn_act_bwd: gz per rank with the GLOBAL sums; dgamma / dbeta this rank's share
        for accumulate in (False, True):
            dgs, dbs = grad_bufs(accumulate)
            first = {"on": True}

            def bwd(k):
                if not first["on"] and accumulate:                     # phase 2 starts from the same values as phase 1
                    dgs[k].t.copy_(f32(acc0)); dbs[k].t.copy_(f32(-acc0))
                return hip.bn_act_bwd(part("z", k), part("ga", k), vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], slope,
                                      dgs[k].t, dbs[k].t, accumulate)
            run = _two_phase(hip, W, bwd, first, b, "sync bn_act_bwd")
            _chk(torch.cat([o[0] for o in run]), X("gz"), fam_b.gz, dtype, "sync.bn_act_bwd.gz", case)
            for k in range(W):
                _chk(run[k][1], X("s_gy"), fam_b.s_gy, torch.float32, "sync.bn_act_bwd.s_gy", case)
                _chk(run[k][2], X("s_gyxh"), fam_b.s_gyxh, torch.float32, "sync.bn_act_bwd.s_gyxh", case)
            a0 = W * acc0 if accumulate else 0.0
            tot_dg, tot_db = rank_sum(dgs), rank_sum(dbs)
            if exact:
                assert torch.equal(tot_dg, fam_x.s_gyxh.v + a0) and torch.equal(tot_db, fam_x.s_gy.v - a0), case + ": dgamma / dbeta"
            else:
                # the ranks' sums are a grouping of the whole batch's: the any-order term of the whole covers them
                _within(tot_dg, B.EV(fam_b.s_gyxh.v + a0, fam_b.s_gyxh.e), torch.float32, "sync.bn_act_bwd.dgamma", case,
                        acc_extra([f.dgamma_local for f in fks]) if accumulate else None)
                _within(tot_db, B.EV(fam_b.s_gy.v - a0, fam_b.s_gy.e), torch.float32, "sync.bn_act_bwd.dbeta", case,
                        acc_extra([f.dbeta_local for f in fks]) if accumulate else None)
        sums_bwd = (run[0][1], run[0][2])
        # ---- bn_tangent
        tan = _two_phase(hip, W, lambda k: hip.bn_tangent(part("z", k), part("zt", k), vec["mean"], vec["invstd"], vec["gamma"],
                                                          vec["beta"], slope), None, b, "sync bn_tangent")
        _chk(torch.cat([o[0] for o in tan]), X("at"), fam_b.at, dtype, "sync.bn_tangent.at", case)
        for k in range(W):
            _chk(tan[k][1], X("s_zt"), fam_b.s_zt, torch.float32, "sync.bn_tangent.s_zt", case)
            _chk(tan[k][2], X("s_xhzt"), fam_b.s_xhzt, torch.float32, "sync.bn_tangent.s_xhzt", case)
        # ---- bn_double_bwd with and without qa: pz with the global coefficients, dgamma = m_LOCAL / sigma (A - b c) + local sums
        for use_qa in (True, False):
            for accumulate in (False, True):
                dgs, dbs = grad_bufs(accumulate)
                first = {"on": True}

                def dbl(k):
                    if not first["on"] and accumulate:
                        dgs[k].t.copy_(f32(acc0)); dbs[k].t.copy_(f32(-acc0))
                    return hip.bn_double_bwd(part("z", k), part("qa", k) if use_qa else None, part("zt", k), part("ga", k),
                                             vec["mean"], vec["invstd"], vec["gamma"], vec["beta"], slope, sums_bwd[0], sums_bwd[1],
                                             tan[0][1], tan[0][2], dgs[k].t, dbs[k].t, accumulate)
                pzs = _two_phase(hip, W, dbl, first, b, "sync bn_double_bwd")
                tag = "%s%s" % ("+qa" if use_qa else "", ".acc" if accumulate else "")
                xd = None if fam_x is None else fam_x.dbl[use_qa]
                _chk(torch.cat(pzs), None if xd is None else xd["pz"], fam_b.dbl[use_qa]["pz"], dtype, "sync.bn_double_bwd.pz" + tag, case)
                a0 = acc0 if accumulate else 0.0
                # rank k's share, from the trees with rows = rank k's: summed over the ranks it is the whole-batch gradient
                tot_dg, tot_db = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
                for k in range(W):
                    dk = fks[k].dbl[use_qa]
                    _chk(dgs[k], B.EV(dk["dg"].v + a0) if exact else None, B.EV(dk["dg"].v + a0, dk["dg"].e), torch.float32,
                         "sync.bn_double_bwd.dgamma" + tag, case + "/rank%d" % k)
                    _chk(dbs[k], B.EV(dk["db"].v - a0) if exact else None, B.EV(dk["db"].v - a0, dk["db"].e), torch.float32,
                         "sync.bn_double_bwd.dbeta" + tag, case + "/rank%d" % k)
                    tot_dg, tot_db = tot_dg + dk["dg"].v, tot_db + dk["db"].v
                whole = fam_b.dbl[use_qa]
                assert torch.allclose(tot_dg, whole["dg"].v, rtol=1e-12, atol=1e-12) and torch.allclose(tot_db, whole["db"].v, rtol=1e-12, atol=1e-12), \
                    "the references' rank shares do not sum to the whole-batch gradient"
        # ---- bn_forward (its split branch): mean / invstd of the whole batch on every rank, a per rank
        z64 = ops["z"]
        rm0 = (0.1 * R.gauss((C,), 23)).float().double()
        rv0 = (1 + 0.1 * R.gauss((C,), 24).abs()).float().double()
        rms, rvs = [b.out((C,), init=rm0) for _ in range(W)], [b.out((C,), init=rv0) for _ in range(W)]
        nbts = [torch.zeros((), dtype=torch.int64, device=DEV) for _ in range(W)]
        first = {"on": True}

        def fwd(k):
            if not first["on"]:
                rms[k].t.copy_(f32(rm0)); rvs[k].t.copy_(f32(rv0)); nbts[k].zero_()
            return hip.bn_forward(part("z", k), vec["gamma"], vec["beta"], slope, EPS, MOM, rms[k].t, rvs[k].t, nbts[k])
        f = _two_phase(hip, W, fwd, first, b, "sync bn_forward")
        r = B.stats_ref(z64, M, EPS, MOM, rm0, rv0)
        for k in range(W):
            _check_stats(case + "/rank%d" % k, "sync.bn_forward", r, f[k][1], f[k][2], rms[k], rvs[k])
            assert int(nbts[k].cpu()) == 1
            assert torch.equal(bits(f[k][1]), bits(f[0][1])) and torch.equal(bits(f[k][2]), bits(f[0][2])), "ranks disagree"
            a_k = hip.bn_act(part("z", k), f[k][1], f[k][2], vec["gamma"], vec["beta"], slope)
            assert torch.equal(_ibits(f[k][0]), _ibits(a_k)), "sync.bn_forward: the activation is not bn_act on the global statistics"
            assert torch.isfinite(f[k][0].float()).all()
        b.check("sync " + case)


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("N,E", [(2, 50), (7, 64), (64, 65), (65, 63)])
def test_sync_latent_prep_and_sqnorm_simulated_ranks(W, N, E):
    """(C) for latent_prep (rg_latent_stats / rg_latent_apply with N_total = W N) and stat_allreduce(sqnorm(.)): reference = the
    whole batch in fp64.  The bound of the split form: its one-pass variance ss - nt mu^2 on fp32 column sums of nt rows.  Every
    rank's part is an allocation of its own inside NaN."""
    env = _Env(torch.float32)
    hip = env.ops
    nt = W * N
    u64, z64 = (0.17 * R.gauss((nt, E), 500 + N)).float().double(), R.gauss((nt, E), 501 + N).float().double()
    b = Bufs()
    us = [b.vec(u64[k * N:(k + 1) * N]) for k in range(W)]
    zs = [b.vec(z64[k * N:(k + 1) * N]) for k in range(W)]
    outs = _two_phase(hip, W, lambda k: hip.latent_prep(us[k].t, zs[k].t), None, b, "sync latent_prep")
    ref, bnd = B.latent_ref(u64, z64, split=True)
    got = torch.cat(outs).cpu().double()
    assert torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / bnd).max())
    print("RATIO sync.latent_prep W%d-%dx%d %.4f" % (W, N, E, ratio))
    assert ratio <= 1.0
    x64 = R.gauss((W, 1027), 510).float().double()
    xs = [b.vec(x64[k]) for k in range(W)]
    sq = _two_phase(hip, W, lambda k: hip.stat_allreduce(hip.sqnorm(xs[k].t)), None, b, "sync sqnorm")
    # the ranks' sums and their all-reduce are one grouping of the sum over all W * 1027 squares: the tree's any-order term
    ctx = B.Ctx(False)
    flat = ctx.leaf(x64.reshape(-1, 1))
    want = ctx.colsum(ctx.mul(flat, flat, "x*x"), "sqnorm over the ranks")
    for k in range(W):
        _within(sq[k], want, torch.float32, "sync.sqnorm", "W%d/rank%d" % (W, k))


# ================================================================== (D) partial-row finishers
G_ALL = [1, 31, 33, 512, 513, 1000, 2052]
M_PART = 4096


def _finalize_checks(case, op, z64, M, rm0, rv0, mean, invstd, rm, rv):
    zero = torch.zeros(z64.shape[1], dtype=torch.float64)
    r = B.stats_ref(z64, M, EPS, MOM, rm0, rv0, zero, zero)           # integer partial rows: every sum in any order is exact
    _equal(mean, r["mean"], torch.float32, "%s.mean[%s]" % (op, case))
    _check_stats(case, op, r, mean, invstd, rm, rv)
    return r


@fp16_twin
@pytest.mark.parametrize("G", G_ALL)
@pytest.mark.parametrize("C", [8, 136, 36])
def test_partial_rows_finalize_and_forward(G, C, h16=torch.bfloat16):
    """(D) rg_bn_finalize_partials and rg_bn_forward_partials on [G][2][C] integer column sums of an integer z [4096][C] cut into
    G row tiles: mean bit-equal, invstd / running statistics within the counted roundings, the activation bit-equal to bn_act on
    the statistics written.  G = 512 / 513 is the switch to the two-level form (C % 8 == 0; per = 17 leaves the last slice
    short), 1000 no multiple of 32; C = 36 stays on the narrow path above G = 512.  The workspace is the header's 32 * 2 * C
    floats: exactly, guarded; partial rows inside NaN."""
    env = _Env(h16)
    lib, dt, st = env.lib, env.dt, env.stream
    M = M_PART
    z64 = B.ints_z(M, C, 600 + G + C)
    part64 = B.partial_rows(z64, G)
    B.partial_condition(part64, z64, M)
    case = "%s/G%d-C%d" % (_name(h16), G, C)
    b = Bufs()
    part = Guarded(part64.float(), NAN, after=512 * 2 * C)
    z = b.operand(z64, h16)
    gamma, beta = b.vec(R.pow2_affine(C, 3)[0]), b.vec(R.pow2_affine(C, 3)[1] * 0.5)
    q = 32 * 2 * C * 4
    ws = b.ws(q)
    rm0, rv0, rm, rv, nbt = _stat_bufs(b, C, 610)
    mean, invstd = b.out((C,)), b.out((C,))
    # one byte less than the header's 32 * 2 * C floats is refused at every G and C: no quiet fall-back to the single-level form
    _refused(env, lib.rg_bn_finalize_partials(_ptr(part), G, M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv), _ptr(nbt),
                                              _ptr(ws), q - 1, st), [mean, invstd, ws], "rg_bn_finalize_partials")
    assert int(nbt.cpu()) == 0 and torch.equal(_cpu(rm).double(), rm0)
    env.ok(lib.rg_bn_finalize_partials(_ptr(part), G, M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv), _ptr(nbt),
                                       _ptr(ws), q, st), "rg_bn_finalize_partials")
    r = _finalize_checks(case, "bn_finalize_partials", z64, M, rm0, rv0, mean, invstd, rm, rv)
    two_level = G > 512 and C % 8 == 0
    assert two_level == (not _untouched(ws, SENTINEL)), "two-level form taken: %s, expected %s" % (not two_level, two_level)
    b.check("bn_finalize_partials")
    # forward: a second update of the running statistics
    mean2, invstd2, a = b.out((C,)), b.out((C,)), b.out((M, C), h16)
    _refused(env, lib.rg_bn_forward_partials(_ptr(part), G, _ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean2),
                                             _ptr(invstd2), _ptr(rm), _ptr(rv), _ptr(nbt), _ptr(a), dt, _ptr(ws), q - 1, st),
             [mean2, invstd2, a], "rg_bn_forward_partials")
    assert int(nbt.cpu()) == 1
    env.ok(lib.rg_bn_forward_partials(_ptr(part), G, _ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean2),
                                      _ptr(invstd2), _ptr(rm), _ptr(rv), _ptr(nbt), _ptr(a), dt, _ptr(ws), q, st),
           "rg_bn_forward_partials")
    assert torch.equal(bits(mean2.t), bits(mean.t)) and torch.equal(bits(invstd2.t), bits(invstd.t))
    zero = torch.zeros(C, dtype=torch.float64)
    r2 = B.stats_ref(z64, M, EPS, MOM, r["rm"], r["rv"], zero, zero)
    r2["e_rm"], r2["e_rv"] = r2["e_rm"] + (1 - MOM) * r["e_rm"], r2["e_rv"] + (1 - MOM) * r["e_rv"]
    _check_stats(case, "bn_forward_partials", r2, mean2, invstd2, rm, rv)
    assert int(nbt.cpu()) == 2
    a_act = b.out((M, C), h16)
    env.ok(lib.rg_bn_act(_ptr(z), _ptr(mean2), _ptr(invstd2), _ptr(gamma), _ptr(beta), _ptr(a_act), M, C, 0.5, dt, st), "rg_bn_act")
    assert torch.equal(_ibits(a.t.clone()), _ibits(a_act.t.clone())), "bn_forward_partials: the activation is not bn_act's"
    assert torch.isfinite(_cpu(a).float()).all()
    b.check("bn_forward_partials")


def _g2_cases():
    out = []
    for nblk in (1, 4):
        for G in G_ALL:
            if G % nblk == 0:
                out.append((G, nblk))
    return out


@fp16_twin
@pytest.mark.parametrize("G,nblk", _g2_cases())
@pytest.mark.parametrize("C", [8, 136, 36])
def test_partial_rows_two_groups(G, nblk, C, h16=torch.bfloat16):
    """(D) rg_bn_finalize_partials_g2 and rg_bn_forward_g2 on the partial rows of two DIFFERENT halves laid out [nblk][2
    halves][G / nblk] (nblk = 4: the transposed conv's class-major rows): per half mean bit-equal and invstd within the counted
    roundings, the running statistics updated by the first half first, then the second (momentum makes the order visible), two
    steps of num_batches_tracked.  Workspaces exactly what HipOps.last_up_bn2 / bn_forward2 pass."""
    env = _Env(h16)
    lib, dt, st = env.lib, env.dt, env.stream
    M = M_PART
    z64 = torch.cat([B.ints_z(M, C, 700 + G + C), B.ints_z(M, C, 701 + G + C, -2, 4) * 2.0])
    part64 = B.partial_rows_g2(z64, G, nblk)
    for h in range(2):
        B.partial_condition(B.partial_rows(z64[h * M:(h + 1) * M], G), z64[h * M:(h + 1) * M], M)
    case = "%s/G%d-nblk%d-C%d" % (_name(h16), G, nblk, C)
    b = Bufs()
    # NaN behind the partial rows for 3 G / nblk + 8 more rows: a row index that forgets the block structure (up to 11 G / 4 - 1 of
    # the 2 G rows) stays inside the allocation and poisons a statistic
    part = Guarded(part64.float(), NAN, after=(3 * G + 8) * 2 * C)
    z = b.operand(z64, h16)
    gamma, beta = b.vec(R.pow2_affine(C, 3)[0]), b.vec(R.pow2_affine(C, 3)[1] * 0.5)
    rm0, rv0, rm, rv, nbt = _stat_bufs(b, C, 710)
    zero = torch.zeros(C, dtype=torch.float64)
    r0 = B.stats_ref(z64[:M], M, EPS, MOM, rm0, rv0, zero, zero)
    r1 = B.stats_ref(z64[M:], M, EPS, MOM, r0["rm"], r0["rv"], zero, zero)
    r1["e_rm"], r1["e_rv"] = r1["e_rm"] + (1 - MOM) * r0["e_rm"], r1["e_rv"] + (1 - MOM) * r0["e_rv"]
    # the other order gives other running statistics: the check below can tell
    o1 = B.stats_ref(z64[M:], M, EPS, MOM, rm0, rv0, zero, zero)
    o0 = B.stats_ref(z64[:M], M, EPS, MOM, o1["rm"], o1["rv"], zero, zero)
    assert bool(((o0["rm"] - r1["rm"]).abs() > 4 * r1["e_rm"]).any()), "the halves are too alike to tell the update order"

    def check(op, mean, invstd, rmv, rvv, r0, r1):
        for h, r in ((0, r0), (1, r1)):
            _equal(mean.t[h], r["mean"], torch.float32, "%s.mean[%s half %d]" % (op, case, h))
            _within(invstd.t[h], B.EV(r["invstd"], r["e_invstd"]), torch.float32, op + ".invstd", case + "/half%d" % h)
        _within(rmv, B.EV(r1["rm"], r1["e_rm"]), torch.float32, op + ".running_mean", case)
        _within(rvv, B.EV(r1["rv"], r1["e_rv"]), torch.float32, op + ".running_var", case)

    q = 2 * 32 * 2 * C * 4
    ws = b.ws(q)
    mean, invstd = b.out((2, C)), b.out((2, C))
    _refused(env, lib.rg_bn_finalize_partials_g2(_ptr(part), G, nblk, M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv),
                                                 _ptr(nbt), _ptr(ws), q - 1, st), [mean, invstd, ws], "rg_bn_finalize_partials_g2")
    assert int(nbt.cpu()) == 0
    env.ok(lib.rg_bn_finalize_partials_g2(_ptr(part), G, nblk, M, C, EPS, MOM, _ptr(mean), _ptr(invstd), _ptr(rm), _ptr(rv),
                                          _ptr(nbt), _ptr(ws), q, st), "rg_bn_finalize_partials_g2")
    check("bn_finalize_partials_g2", mean, invstd, rm, rv, r0, r1)
    assert int(nbt.cpu()) == 2
    assert (G > 512 and C % 8 == 0) == (not _untouched(ws, SENTINEL))
    b.check("bn_finalize_partials_g2")
    # forward: third and fourth update
    r2 = B.stats_ref(z64[:M], M, EPS, MOM, r1["rm"], r1["rv"], zero, zero)
    r3 = B.stats_ref(z64[M:], M, EPS, MOM, r2["rm"], r2["rv"], zero, zero)
    r2["e_rm"], r2["e_rv"] = r2["e_rm"] + (1 - MOM) * r1["e_rm"], r2["e_rv"] + (1 - MOM) * r1["e_rv"]
    r3["e_rm"], r3["e_rv"] = r3["e_rm"] + (1 - MOM) * r2["e_rm"], r3["e_rv"] + (1 - MOM) * r2["e_rv"]
    qf = 2 * lib.rg_colreduce_workspace_bytes(M, C, 2) + 2 * 32 * 2 * C * 4
    wsf = b.ws(qf)
    mean2, invstd2, a = b.out((2, C)), b.out((2, C)), b.out((2 * M, C), h16)
    _refused(env, lib.rg_bn_forward_g2(_ptr(part), G, nblk, _ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean2),
                                       _ptr(invstd2), _ptr(rm), _ptr(rv), _ptr(nbt), _ptr(a), dt, _ptr(wsf), q - 1, st),
             [mean2, invstd2, a, wsf], "rg_bn_forward_g2 (partial rows)")
    assert int(nbt.cpu()) == 2
    env.ok(lib.rg_bn_forward_g2(_ptr(part), G, nblk, _ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean2),
                                _ptr(invstd2), _ptr(rm), _ptr(rv), _ptr(nbt), _ptr(a), dt, _ptr(wsf), qf, st), "rg_bn_forward_g2")
    assert torch.equal(bits(mean2.t), bits(mean.t)) and torch.equal(bits(invstd2.t), bits(invstd.t))
    check("bn_forward_g2", mean2, invstd2, rm, rv, r2, r3)
    assert int(nbt.cpu()) == 4
    for h in range(2):
        zh = b.operand(z64[h * M:(h + 1) * M], h16)
        mh, ih = b.vec(_cpu(mean2.t[h]).double()), b.vec(_cpu(invstd2.t[h]).double())
        a_act = b.out((M, C), h16)
        env.ok(lib.rg_bn_act(_ptr(zh), _ptr(mh), _ptr(ih), _ptr(gamma), _ptr(beta), _ptr(a_act), M, C, 0.5, dt, st), "rg_bn_act")
        assert torch.equal(_ibits(a.t[h * M:(h + 1) * M].clone()), _ibits(a_act.t.clone())), "bn_forward_g2: half %d is not bn_act's" % h
    b.check("bn_forward_g2")
    if G == 33:
        # no partial rows: the statistics pass over z itself, two groups (gridDim.z = 2)
        rm2, rv2 = b.out((C,), init=rm0), b.out((C,), init=rv0)
        mean3, invstd3, a3 = b.out((2, C)), b.out((2, C)), b.out((2 * M, C), h16)
        fa = lambda nbytes: (0, 0, 1, _ptr(z), M, C, EPS, MOM, _ptr(gamma), _ptr(beta), 0.5, _ptr(mean3), _ptr(invstd3), _ptr(rm2),
                             _ptr(rv2), _ptr(nbt), _ptr(a3), dt, _ptr(wsf), nbytes, st)
        _refused(env, lib.rg_bn_forward_g2(*fa(2 * lib.rg_colreduce_workspace_bytes(M, C, 2) - 1)), [mean3, invstd3, a3], "rg_bn_forward_g2")
        env.ok(lib.rg_bn_forward_g2(*fa(qf)), "rg_bn_forward_g2")
        check("bn_forward_g2(z)", mean3, invstd3, rm2, rv2, r0, r1)
        assert torch.equal(_ibits(a3.t.clone()), _ibits(a.t.clone()))
        b.check("bn_forward_g2(z)")


# ================================================================== rg_misc.hip
MISC_N = [1, 3, 4, 255, 257, 1027, 1024 * 256 + 5]


@pytest.mark.parametrize("n", MISC_N)
def test_misc_elementwise(n):
    """tanh_bwd, interp (host eps and rg_interp_dev), scale_by, clamp_ at sizes that reach the float4 body alone (4), the tail
    alone (1, 3) and both, and one above RED_BLOCKS * 256.  (A): dyadic operands make every product and sum exact, the result is
    bit-equal.  (B): Gaussian operands, bound = the counted roundings of each functor."""
    env = _Env(torch.float32)
    lib, st = env.lib, env.stream
    case = "n%d" % n
    f = lambda t: t.float().double()
    for kind in ("E", "B"):
        if kind == "E":
            gy, y = R.ints((n,), 1, -4, 4), R.ints((n,), 2, -4, 4) * 0.25
            real, fake, eps = R.ints((n,), 3, -8, 8), R.ints((n,), 4, -8, 8), 0.25
            coef = torch.tensor([-0.5], dtype=torch.float64)
        else:
            gy, y = f(R.gauss((n,), 1)), f(torch.tanh(R.gauss((n,), 2)))
            real, fake, eps = f(R.gauss((n,), 3)), f(R.gauss((n,), 4)), 0.37
            coef = f(torch.tensor([1.7], dtype=torch.float64) / 3)
        ctx = B.Ctx(kind == "E")
        L = ctx.leaf
        b = Bufs()
        g_gy, g_y, g_real, g_fake, g_coef = (b.vec(t) for t in (gy, y, real, fake, coef))
        # TanhBwd: g * (1 - v * v): 3 roundings
        out = b.out((n,))
        env.ok(lib.rg_tanh_bwd(_ptr(g_gy), _ptr(g_y), _ptr(out), n, st), "rg_tanh_bwd")
        tree = ctx.mul(L(gy), ctx.sub(L(1.0), ctx.mul(L(y), L(y))))
        _chk(out, tree if kind == "E" else None, tree, torch.float32, "tanh_bwd", case + kind)
        # Interp: e * a + (1 - e) * b: e1 = 1 - e [1], two products [2], the sum [1]; the store adds none (fp32)
        e32 = float(np.float32(eps))
        e1 = ctx.sub(L(1.0), L(e32))
        tree = ctx.add(ctx.mul(L(e32), L(real)), ctx.mul(e1, L(fake)))
        for dev_eps in (False, True):
            out = b.out((n,))
            if dev_eps:
                g_eps = b.vec(torch.tensor([e32], dtype=torch.float64))
                env.ok(lib.rg_interp_dev(_ptr(g_real), _ptr(g_fake), _ptr(out), n, _ptr(g_eps), st), "rg_interp_dev")
            else:
                env.ok(lib.rg_interp(_ptr(g_real), _ptr(g_fake), _ptr(out), n, e32, st), "rg_interp")
            _chk(out, tree if kind == "E" else None, tree, torch.float32, "interp_dev" if dev_eps else "interp", case + kind)
        # ScaleBy: one product
        out = b.out((n,))
        env.ok(lib.rg_scale_by(_ptr(g_real), _ptr(g_coef), _ptr(out), n, st), "rg_scale_by")
        tree = ctx.mul(L(real), L(coef))
        _equal(out, tree.v, torch.float32, "scale_by[%s]" % case)     # a single correctly rounded product in both kinds
        # Clamp, in place: no arithmetic, bit-equal
        p = b.out((n,), init=real)
        env.ok(lib.rg_clamp(_ptr(p), n, -0.5, 0.75, st), "rg_clamp")
        _equal(p, real.clamp(-0.5, 0.75), torch.float32, "clamp[%s]" % case)
        b.check("misc element-wise " + case)


@pytest.mark.parametrize("n", MISC_N)
def test_misc_scalar_reductions(n):
    """sqnorm, mean_diff (with and without b), vec_sum (written and accumulated), gp_coef.  (A): integer operands, the sum is exact
    and must be bit-equal in any order.  (B): Gaussian operands, (n - 1) 2^-24 sum |t| for the any-order summation plus each
    term's own roundings.  The workspace of sqnorm is exactly rg_reduce_workspace_bytes inside guards; one byte less is refused."""
    env = _Env(torch.float32)
    lib, st = env.lib, env.stream
    case = "n%d" % n
    for kind in ("E", "B"):
        exact = kind == "E"
        x = R.ints((n,), 11, -3, 3) if exact else R.gauss((n,), 11).float().double()
        y = R.ints((n,), 12, -3, 3) if exact else R.gauss((n,), 12).float().double()
        ctx = B.Ctx(exact)
        L = ctx.leaf
        b = Bufs()
        gx, gy = b.vec(x), b.vec(y)
        col = lambda ev: ctx.colsum(B.EV(ev.v[:, None], ev.e[:, None]))
        # sqnorm
        q = lib.rg_reduce_workspace_bytes(n)
        ws = b.ws(q)
        out = b.out((1,))
        _refused(env, lib.rg_sqnorm(_ptr(gx), _ptr(out), n, _ptr(ws), q - 1, st), [out, ws], "rg_sqnorm")
        env.ok(lib.rg_sqnorm(_ptr(gx), _ptr(out), n, _ptr(ws), q, st), "rg_sqnorm")
        sq = col(ctx.mul(L(x), L(x)))
        _chk(out, sq if exact else None, sq, torch.float32, "sqnorm", case + kind)
        # mean_diff: sign * sum / n: the difference [1], the sum, the product with sign [exact: +-1], the division [1]
        for use_b in (True, False):
            out = b.out((1,))
            env.ok(lib.rg_mean_diff(_ptr(gx), _ptr(gy) if use_b else 0, _ptr(out), n, -1.0, st), "rg_mean_diff")
            t = col(ctx.sub(L(x), L(y)) if use_b else L(x))
            ref = B.EV(-t.v / n, t.e / n + U32 * (t.v.abs() + t.e) / n)
            if exact and (n & (n - 1)) == 0:
                _equal(out, ref.v, torch.float32, "mean_diff[%s]" % case)
            else:
                _within(out, ref, torch.float32, "mean_diff" + ("" if use_b else "(a)"), case + kind)
        # vec_sum
        for accumulate in (0, 1):
            out = b.out((1,), init=torch.tensor([5.0], dtype=torch.float64)) if accumulate else b.out((1,))
            env.ok(lib.rg_vec_sum(_ptr(gx), n, _ptr(out), accumulate, st), "rg_vec_sum")
            t = col(L(x))
            t = B.EV(t.v + (5.0 if accumulate else 0.0), t.e)
            _chk(out, t if exact else None, t, torch.float32, "vec_sum" + (".acc" if accumulate else ""), case + kind)
        b.check("misc reductions " + case)
    # gp_coef: the counted roundings of _gp_ref; exact at sq = 1/4 and 4
    for sqv in (0.25, 4.0, 1.7, 1.0 + 2.0 ** -10):
        b = Bufs()
        g_sq = b.vec(torch.tensor([sqv], dtype=torch.float64))
        loss, coef = b.out((1,)), b.out((1,))
        env.ok(lib.rg_gp_coef(_ptr(g_sq), _ptr(loss), _ptr(coef), 10.0, st), "rg_gp_coef")
        rl, el, rc, ec = _gp_ref(float(np.float32(sqv)), 0.0, 10.0)
        if sqv in (0.25, 4.0):
            assert float(loss.t) == rl and float(coef.t) == rc, "gp_coef at sq = %g (exact)" % sqv
        _within(loss, B.EV(torch.tensor([rl], dtype=torch.float64), torch.tensor([el], dtype=torch.float64)), torch.float32, "gp_coef.loss", "sq%g" % sqv)
        _within(coef, B.EV(torch.tensor([rc], dtype=torch.float64), torch.tensor([ec], dtype=torch.float64)), torch.float32, "gp_coef.coef", "sq%g" % sqv)
        b.check("gp_coef")


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("HW", [15, 1024])
def test_nchw_chan_sum(N, C, HW):
    """out[c] (+)= sum over n, hw of g[n][c][hw] in 256 chunks per channel: (A) integers, bit-equal; (B) Gaussian, any-order
    bound; written and accumulated; the workspace exactly C * 256 floats inside guards, one byte less refused."""
    env = _Env(torch.float32)
    lib, st = env.lib, env.stream
    case = "%dx%dx%d" % (N, C, HW)
    for exact in (True, False):
        g64 = R.ints((N, C, HW), 21, -3, 3) if exact else R.gauss((N, C, HW), 21).float().double()
        ctx = B.Ctx(exact)
        t = ctx.colsum(ctx.leaf(g64.permute(0, 2, 1).reshape(N * HW, C)))
        b = Bufs()
        g = b.vec(g64)
        q = C * 256 * 4
        ws = b.ws(q)
        for accumulate in (0, 1):
            a0 = R.ints((C,), 22, -5, 5)
            out = b.out((C,), init=a0) if accumulate else b.out((C,))
            if not accumulate:
                _refused(env, lib.rg_nchw_chan_sum(_ptr(g), _ptr(out), N, C, HW, 0, _ptr(ws), q - 1, st), [out, ws], "rg_nchw_chan_sum")
            env.ok(lib.rg_nchw_chan_sum(_ptr(g), _ptr(out), N, C, HW, accumulate, _ptr(ws), q, st), "rg_nchw_chan_sum")
            ref = B.EV(t.v + (a0 if accumulate else 0.0), t.e)
            _chk(out, ref if exact else None, ref, torch.float32, "nchw_chan_sum" + (".acc" if accumulate else ""),
                 case + ("E" if exact else "B"))
            b.check("nchw_chan_sum")


@pytest.mark.parametrize("N", [2, 7, 64, 65])
@pytest.mark.parametrize("E", [50, 63, 64, 65])
def test_latent_prep(N, E):
    """(v - mean) / std over the N rows of v = u + z, unbiased std: N <= 64 the register kernel, 65 the three-pass kernel; E
    around the 64-column block.  Bound from the counted roundings of the two-pass form (bn_reduce_refs.latent_ref)."""
    env = _Env(torch.float32)
    lib, st = env.lib, env.stream
    u64, z64 = (0.17 * R.gauss((N, E), 35)).float().double(), R.gauss((N, E), 36).float().double()
    b = Bufs()
    u, z = b.vec(u64), b.vec(z64)
    out = b.out((N, E))
    env.ok(lib.rg_latent_prep(_ptr(u), _ptr(z), _ptr(out), N, E, st), "rg_latent_prep")
    ref, bnd = B.latent_ref(u64, z64, split=False)
    got = _cpu(out).double()
    assert torch.isfinite(got).all()
    ratio = float(((got - ref).abs() / bnd).max())
    print("RATIO latent_prep %dx%d %.4f" % (N, E, ratio))
    assert ratio <= 1.0
    b.check("latent_prep")


@pytest.mark.parametrize("nb", [1, 7, 256, 300])
def test_parts_chan_sum_and_gp_coef_parts(nb):
    """parts [nb][4] (three channel sums and a sum of squares per workgroup of rg_last_up_post): out[c] (+)= sum over the rows,
    gp_coef_parts = gp_coef on the sum of column 3.  Integer rows: bit-equal; the squared norm is chosen a perfect square, so
    that loss and coef are exact as well."""
    env = _Env(torch.float32)
    hip = env.ops
    parts64 = R.ints((nb, 4), 31, -3, 3)
    parts64[:, 3] = 0.0
    parts64[0, 3] = 4.0 if nb == 1 else 1.0
    if nb > 1:
        parts64[nb - 1, 3] = 3.0                                        # sum 4: norm 2, loss 1, coef 10 * 2 * 1 / 2 = 10
    g = Guarded(parts64.float(), NAN)
    a0 = R.ints((3,), 32, -5, 5)
    for accumulate in (False, True):
        out = Guarded(a0.float() if accumulate else torch.full((3,), SENTINEL), SENTINEL)
        hip.parts_chan_sum(g.t, out.t, accumulate)
        torch.cuda.synchronize()
        _equal(out, parts64[:, :3].sum(0) + (a0 if accumulate else 0.0), torch.float32, "parts_chan_sum[nb=%d]" % nb)
        assert out.surroundings_keep(SBITS)
    scale = hip.gp_seed_scale * hip.gp_tangent_scale
    loss, coef = hip.gp_coef_parts(g.t, 10.0)
    torch.cuda.synchronize()
    assert float(loss.cpu()) == 1.0 and float(coef.cpu()) == 10.0 * scale, (float(loss.cpu()), float(coef.cpu()))


# ================================================================== rg_last_up_pre's statistics source
@fp16_twin
@pytest.mark.parametrize("form", ["last_up_bn", "last_up_bn2"])
def test_last_up_bn_statistics_source(form, h16=torch.bfloat16):
    """HipOps.last_up_bn / last_up_bn2 (rg_bn_finalize_partials / _g2 with nblk = 4 -> rg_last_up_pre) at the smallest shape
    rg_last_up_pre_supported accepts: 16-bit storage, O = 64, Wo = 32, I = 3; n = 2 images of 8 rows per batch half (M = 512, a
    power of two; G = 36 partial rows: two rounds of the finisher's lanes, a multiple of nblk).  Reference: last_up(bn_act(z)) in
    fp64 on the statistics of the partial rows.  Bound, per output: the BatchNorm tree's bound of a (mean / invstd carrying the
    finisher's roundings) plus one 16-bit unit of a (the staged row is a matrix-core operand), carried through |w|; K + 1 = 4 O + 1
    fp32 roundings of sum |a||w| + |bias| (any-order accumulation and the bias); tanh is 1-Lipschitz and adds 1 ulp = 2 units.
    The second half of last_up_bn2 has statistics of its own, and the running statistics see the first half first."""
    from types import SimpleNamespace
    from oracle.ops_ref import RefOps
    from rna_gan_amd.engine import ConvW
    env = _Env(h16)
    hip, lib = env.ops, env.lib
    n, Ho, Wo, O, I, G = 2, 8, 32, 64, 3, 36
    assert lib.rg_last_up_pre_supported(Wo, O, I, env.dt)
    assert not lib.rg_last_up_pre_supported(16, O, I, env.dt) and not lib.rg_last_up_pre_supported(Wo, 32, I, env.dt)
    groups = 2 if form == "last_up_bn2" else 1
    M = n * Ho * Wo
    z64 = B.ints_z(M, O, 800)
    if groups == 2:
        z64 = torch.cat([z64, B.ints_z(M, O, 801, -2, 4) * 2.0])
    part64 = B.partial_rows(z64, G) if groups == 1 else B.partial_rows_g2(z64, G, 4)
    for h in range(groups):
        B.partial_condition(B.partial_rows(z64[h * M:(h + 1) * M], G), z64[h * M:(h + 1) * M], M)
    w64 = (0.2 * R.gauss((O, I, 4, 4), 802)).float().to(h16).double()             # weights the storage type holds
    bias64 = (0.1 * R.gauss((I,), 803)).float().double()
    gamma64, beta64 = (1 + 0.1 * R.gauss((O,), 804)).float().double(), (0.1 * R.gauss((O,), 805)).float().double()
    b = Bufs()
    z = b.operand(z64.reshape(groups * n, Ho, Wo, O), h16)
    part = Guarded(part64.float(), NAN, after=(3 * G + 8) * 2 * O)
    gamma, beta, w, bias = b.vec(gamma64), b.vec(beta64), b.vec(w64), b.vec(bias64)
    rm0, rv0, rm, rv, nbt = _stat_bufs(b, O, 810)
    bn = SimpleNamespace(running_mean=rm.t, running_var=rv.t, nbt=nbt[0], eps=EPS, momentum=MOM, gamma=gamma.t, beta=beta.t)
    cw = ConvW(w.t, None)
    ref64 = RefOps(torch.float64)
    zero = torch.zeros(O, dtype=torch.float64)
    slope = 0.2
    # ---- the reference and its bound, per half
    pre, err, stats = [], [], []
    rmp, rvp = rm0, rv0
    for h in range(groups):
        zh = z64[h * M:(h + 1) * M]
        r = B.stats_ref(zh, M, EPS, MOM, rmp, rvp, zero, zero)
        rmp, rvp = r["rm"], r["rv"]
        stats.append(r)
        ctx = B.Ctx(False)
        p = B.P(ctx, r["mean"], r["invstd"].float().double(), gamma64, beta64, slope)
        p.mean, p.rstd = ctx.leaf(r["mean"], r["e_mean"]), ctx.leaf(r["invstd"], r["e_invstd"])
        a, _ = B.bn_act_tree(ctx, ctx.leaf(zh), p)
        e_a = a.e + B.UNIT[h16] * (a.v.abs() + a.e)
        nh = lambda t: t.reshape(n, Ho, Wo, O)
        pre.append(ref64.last_up(nh(a.v), ConvW(w64, None), bias64, False))
        S = ref64.last_up(nh(a.v.abs() + e_a), ConvW(w64.abs(), None), bias64.abs(), False)
        err.append(ref64.last_up(nh(e_a), ConvW(w64.abs(), None), None, False) + (4 * O + 1) * U32 * S)
    pre, err = torch.cat(pre), torch.cat(err)
    fn = getattr(hip, form)
    for tanh in (False, True):
        y = fn(z.t, part.t, bn, slope, cw, bias.t, tanh, update_running=not tanh)
        torch.cuda.synchronize()
        assert y is not None and tuple(y.shape) == (groups * n, I, 2 * Ho, 2 * Wo)
        got = y.cpu().double()
        assert torch.isfinite(got).all(), form + ": non-finite output (a guard region was read?)"
        ref = torch.tanh(pre) if tanh else pre
        bnd = err + (3 if tanh else 1) * U32 * ref.abs()
        ratio = float(((got - ref).abs() / bnd).max())
        print("RATIO %s%s %s/2x8x32x64 %.4f" % (form, ".tanh" if tanh else "", _name(h16), ratio))
        assert ratio <= 1.0, "%s: worst |err| / bound %.2f" % (form, ratio)
        b.check(form)
    # the running statistics: one update per half (the call with update_running=False left them alone), first half first
    last = stats[-1]
    e_rm, e_rv = last["e_rm"], last["e_rv"]
    if groups == 2:
        e_rm, e_rv = e_rm + (1 - MOM) * stats[0]["e_rm"], e_rv + (1 - MOM) * stats[0]["e_rv"]
    _within(rm, B.EV(last["rm"], e_rm), torch.float32, form + ".running_mean", _name(h16))
    _within(rv, B.EV(last["rv"], e_rv), torch.float32, form + ".running_var", _name(h16))
    assert int(nbt.cpu()) == groups


def _gp_ref(sq, e_sq, lambd):
    """gp_coef_kernel: nrm = sqrtf(sq) [1]; loss = (nrm - 1)^2 [2]; coef = lambd * 2 * (nrm - 1) / nrm [the difference, a
    product, the division at 1 ulp = 2 units: 3 of the result]: (loss, e_loss, coef, e_coef) from sq +- e_sq"""
    nrm = sq ** 0.5
    e_n = e_sq / (2 * (sq - e_sq) ** 0.5) + U32 * nrm
    d, e_d = nrm - 1.0, e_n + U32 * abs(nrm - 1.0)
    loss, e_loss = d * d, 2 * abs(d) * e_d + e_d * e_d + U32 * d * d
    coef = 2 * lambd * d / nrm
    return loss, e_loss, coef, 2 * lambd * (e_d / (nrm - e_n) + abs(d) * e_n / (nrm * (nrm - e_n))) + 3 * U32 * abs(coef)


@pytest.mark.parametrize("nb", [1, 7, 256, 300])
def test_parts_chan_sum_and_gp_coef_parts_bound(nb):
    """(B) for the two consumers of rg_last_up_post's partial rows: Gaussian channel sums, squares in column 3; any-order
    summation bound over the nb rows, gp_coef's counted roundings on top of the bound of the squared norm."""
    env = _Env(torch.float32)
    hip = env.ops
    parts64 = R.gauss((nb, 4), 41).float().double()
    parts64[:, 3] = (parts64[:, 3] ** 2 + 0.5).float().double()
    g = Guarded(parts64.float(), NAN)
    ctx = B.Ctx(False)
    t = ctx.colsum(ctx.leaf(parts64))
    a0 = R.ints((3,), 32, -5, 5)
    for accumulate in (False, True):
        out = Guarded(a0.float() if accumulate else torch.full((3,), SENTINEL), SENTINEL)
        hip.parts_chan_sum(g.t, out.t, accumulate)
        torch.cuda.synchronize()
        _within(out, B.EV(t.v[:3] + (a0 if accumulate else 0.0), t.e[:3]), torch.float32,
                "parts_chan_sum" + (".acc" if accumulate else ""), "nb%d" % nb)
        assert out.surroundings_keep(SBITS)
    scale = hip.gp_seed_scale * hip.gp_tangent_scale
    loss, coef = hip.gp_coef_parts(g.t, 10.0)
    torch.cuda.synchronize()
    rl, el, rc, ec = _gp_ref(float(t.v[3]), float(t.e[3]), 10.0)
    T = lambda v: torch.tensor([v], dtype=torch.float64)
    _within(loss, B.EV(T(rl), T(el)), torch.float32, "gp_coef_parts.loss", "nb%d" % nb)
    _within(coef, B.EV(T(rc * scale), T(ec * scale)), torch.float32, "gp_coef_parts.coef", "nb%d" % nb)
