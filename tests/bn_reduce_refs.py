"""fp64 references and operand builders of tests/test_bn_reduce_ops_gpu.py (the row-loop kernels of rg_bn.hip and the small
reductions / element-wise kernels of rg_misc.hip, op by op).

Everything here runs on the CPU in torch fp64 and takes nothing from rna_gan_amd; tests/test_bn_reduce_refs_cpu.py pins each
reference against torch autograd in fp64 and asserts the exactness and non-triviality conditions of the GPU cases on the same
operands, so that the conditions are checked without a kernel.

THE EXPRESSION TREES.  Each kernel expression is written out once, from its functor, ONE NODE PER fp32 ROUNDING, on values that
carry a worst-case error bound next to the fp64 value (class Ctx):
    exact mode   every node must survive a round trip through fp32 (asserted); the result is then what the kernel must store,
                 rounded once to the output type;
    bound mode   every node adds one rounding unit 2^-24 of its own magnitude to the first-order propagated error of its
                 inputs (|a| e_b + |b| e_a + e_a e_b for a product, e_a + e_b for a sum), a column sum adds the any-order
                 summation term (M - 1) 2^-24 sum |t_i|, the store adds one unit of the storage type.  The bound of an element is
                 therefore its count of roundings, each weighed by the magnitude it acts on -- nothing in it is measured.
A fused multiply-add rounds once where the tree rounds twice: its result lies inside the same bound, and in exact mode every
intermediate is exact either way.  The LeakyReLU mask is a comparison: its operand y must be farther from zero than its own
error bound (a CONDITION of a bound-mode case, asserted on the reference), except where y == 0 exactly in exact mode, where the
mask is `slope` (torch's convention, oracle.ops_ref._lrelu_mask's and the kernels' lrelu_mask).
"""
import torch

from vae_fid_refs import U32, gauss

UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # unit round-off of a storage type


# ------------------------------------------------------------------ make_plan of rg_bn.hip, mirrored
def make_plan(M, C, esize, target=1536, gy_cap=512):
    """rg_bn.hip make_plan<T>(M, C, target, gy_cap): esize = sizeof(T); target 1536 (reductions) / 4096, cap 8192 (applies)"""
    vmax = 8 if esize == 2 else 4
    vec = vmax if C % vmax == 0 else (4 if C % 4 == 0 else 1)
    cvec = -(-C // vec)
    tx = 32 if cvec >= 32 else (16 if cvec >= 16 else 8)
    gx = -(-cvec // tx)
    ty = 256 // tx
    want, maxg = -(-target // gx), -(-M // (4 * ty))
    gy = min(max(min(want, maxg), 1), gy_cap)
    rpb = -(-M // gy)
    gy = -(-M // rpb)
    return {"vec": vec, "tx": tx, "ty": ty, "gx": gx, "gy": gy, "rpb": rpb, "last": M - (gy - 1) * rpb,
            "ragged_cols": gx * tx * vec > C + (tx - 1) * vec if gx > 1 else False}


def plan_id(M, C, esize):
    p = make_plan(M, C, esize)
    # unrolled: does any thread of the reduction run its U = 4 body (r + 3 TY < r1), or the remainder loop alone?
    unrolled = p["rpb"] > 3 * p["ty"]
    return "M%dxC%d-vec%d-tx%d-gx%d-gy%d-last%d-%s" % (M, C, p["vec"], p["tx"], p["gx"], p["gy"], p["last"],
                                                      "unroll" if unrolled else "remainder")


# M x C of part A.  Every value of every plan field with both element sizes (asserted in the CPU file): vec 8 / 4 / 1, tx 8 / 16 /
# 32, gx = 2 with a partly empty second column block, gy = 33 with a 7-row last block (1031 rows, C >= 37), the remainder loop
# alone (M = 1, 37).  C = 68 is not in the issue's list: it is the fp32 shape with tx = 16 (cvec = 17), which that list lacks.
PLAN_CASES = [(1, 37), (1, 264), (37, 6), (37, 8), (64, 12), (64, 68), (1024, 36), (1031, 37), (1024, 136), (1031, 264), (64, 264),
              (1031, 136), (1031, 68)]
EXACT_SEED = {(37, 8): 2, (64, 12): 8}         # the first seed of exact_operands at which every condition of part A holds (default 1)
FUSED_CASES = {2: [(64, 256), (300, 256)], 4: [(64, 128), (300, 128)]}      # RNAGAN_BN_FUSED=1: C / vec >= 32, M >= 64


# ------------------------------------------------------------------ values with a running error bound
class EV:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e


class Ctx:
    """exact = True: every node must be an fp32 number (asserted) and carries no error.  exact = False: see the module text."""

    def __init__(self, exact, y_exact=False, strict_leaves=True):
        self.exact = exact
        self.strict_leaves = strict_leaves      # False only where the CPU file pins the trees against autograd on fp64 operands
        self.y_exact = y_exact          # bound mode on the exact operands of part A: y is exact, the mask decided (y == 0 too)
        self.nodes = 0

    def leaf(self, v, e=None):
        v = torch.as_tensor(v, dtype=torch.float64)
        assert not self.strict_leaves or torch.equal(v.float().double(), v) or e is not None, "a leaf that is not an fp32 number needs an error bound"
        return EV(v, None if e is None else torch.as_tensor(e, dtype=torch.float64) + torch.zeros_like(v))

    def _round(self, v, e, what):
        self.nodes += 1
        if self.exact:
            assert torch.equal(v.float().double(), v), "%s: node %d does not survive a round trip through fp32" % (what, self.nodes)
            assert not bool(e.any()), what
            return EV(v, e)
        return EV(v, e + U32 * (v.abs() + e))

    def add(self, a, b, what="add"):
        return self._round(a.v + b.v, a.e + b.e, what)

    def sub(self, a, b, what="sub"):
        return self._round(a.v - b.v, a.e + b.e, what)

    def mul(self, a, b, what="mul"):
        return self._round(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e, what)

    def neg(self, a):
        return EV(-a.v, a.e)

    def colsum(self, t, what="colsum"):
        """sum over the rows in ANY order and grouping: (M - 1) roundings on the longest path, each at most a unit of sum |t|"""
        M = t.v.shape[0]
        S = (t.v.abs() + t.e).sum(0)
        v, e = t.v.sum(0), t.e.sum(0)
        if self.exact:
            assert float(S.max()) <= 2 ** 24 * float(_quantum(t.v)), "%s: partial sums leave fp32's exact range" % what
            assert torch.equal(v.float().double(), v) and not bool(e.any()), what
            return EV(v, e)
        g = (M - 1) * U32
        return EV(v, e + g / (1 - g) * S)

    def mask(self, y, slope, what="mask"):
        """lrelu_mask(y, slope) = y > 0 ? 1 : slope; y == 0 takes slope.  In bound mode the comparison must be decided."""
        if not self.exact and not self.y_exact:
            assert bool((y.v.abs() > y.e).all()), "%s: %d elements whose sign the rounding could flip (change the seed)" % (
                what, int((y.v.abs() <= y.e).sum()))
        return EV(torch.where(y.v > 0, torch.ones_like(y.v), torch.full_like(y.v, slope)))


def _quantum(v):
    """the largest power of two that divides every entry (entries are dyadic rationals): sums of multiples of q are exact in
    fp32 while sum |t| <= 2^24 q"""
    nz = v[v != 0].abs()
    if nz.numel() == 0:
        return 1.0
    q = 1.0
    while bool((torch.round(nz / q) != nz / q).any()):
        q /= 2
        assert q > 2.0 ** -40
    return q


HALF_STEP = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}   # half the subnormal spacing


def store_bound(x, dtype):
    """(reference, bound) of x rounded once to `dtype`: one unit of the value, or half a subnormal step where the format has
    run out of exponent (fp16 below 2^-14: a Gaussian case has a few such elements next to y = 0)"""
    return x.v, x.e + torch.clamp(UNIT[dtype] * (x.v.abs() + x.e), min=HALF_STEP[dtype])


# ------------------------------------------------------------------ the functors of rg_bn.hip
class P:
    """per-channel parameters as leaves (BNC / BNR): mean, rstd, gam, bet [C], slope"""

    def __init__(self, ctx, mean, invstd, gamma, beta, slope):
        self.mean, self.rstd, self.gam, self.bet = (ctx.leaf(t) for t in (mean, invstd, gamma, beta))
        self.slope = float(torch.tensor(slope, dtype=torch.float32))          # the kernels take a float


def _xh_y(ctx, z, p):
    # BwdRedF / BwdApplyF / TanRedF / DblRedF: xh = (z - mean) * rstd [2 roundings]; y = xh * gam + bet [2]
    xh = ctx.mul(ctx.sub(z, p.mean, "z-mean"), p.rstd, "xh")
    y = ctx.add(ctx.mul(xh, p.gam, "xh*gam"), p.bet, "y")
    return xh, y


def bn_act_tree(ctx, z, p):
    """BnActF::finish: lrelu_f((z - mean) * (rstd * gam) + bet, slope): 4 roundings, a 5th where y <= 0 and slope != 0, 1"""
    y = ctx.add(ctx.mul(ctx.sub(z, p.mean, "z-mean"), ctx.mul(p.rstd, p.gam, "rstd*gam"), "prod"), p.bet, "y")
    neg = ctx.mul(y, ctx.leaf(p.slope), "y*slope")
    if not ctx.exact and not ctx.y_exact:
        assert bool((y.v.abs() > y.e).all()), "bn_act: an element whose sign the rounding could flip"
    pos = y.v > 0
    return EV(torch.where(pos, y.v, neg.v), torch.where(pos, y.e, neg.e)), y


def bwd_terms(ctx, z, ga, p):
    """BwdRedF::accum: gy = ga * mask [1], gy * xh [1] -> the terms of s_gy, s_gyxh"""
    xh, y = _xh_y(ctx, z, p)
    mk = ctx.mask(y, p.slope, "bwd mask")
    gy = ctx.mul(ga, mk, "gy")
    return xh, y, mk, gy, ctx.mul(gy, xh, "gy*xh")


def bwd_apply_tree(ctx, xh, gy, p, s_gy, s_gyxh, inv_m):
    """BwdApplyF: m1 = s_gy * inv_m [1], m2 = s_gyxh * inv_m [1]; o = (gam * rstd) * (gy - m1 - xh * m2) [1 + 1 + 1 + 1 + 1]
    on top of xh [2] and gy [1]: 10 roundings, + inv_m's own when M is no power of two"""
    m1, m2 = ctx.mul(s_gy, inv_m, "m1"), ctx.mul(s_gyxh, inv_m, "m2")
    inner = ctx.sub(ctx.sub(gy, m1, "gy-m1"), ctx.mul(xh, m2, "xh*m2"), "inner")
    return ctx.mul(ctx.mul(p.gam, p.rstd, "gam*rstd"), inner, "gz")


def tan_terms(ctx, z, zt, p):
    """TanRedF::accum: the terms of s_zt (zt itself) and s_xhzt = xh * zt [2 + 1]"""
    xh, y = _xh_y(ctx, z, p)
    return xh, y, ctx.mul(xh, zt, "xh*zt")


def tan_apply_tree(ctx, xh, y, zt, p, s_zt, s_xhzt, inv_m):
    """TanApplyF: yt = (gam * rstd) * (zt - m1 - xh * m2); o = yt * mask: 11 roundings with xh's two"""
    m1, m2 = ctx.mul(s_zt, inv_m, "m1"), ctx.mul(s_xhzt, inv_m, "m2")
    inner = ctx.sub(ctx.sub(zt, m1, "zt-m1"), ctx.mul(xh, m2, "xh*m2"), "inner")
    yt = ctx.mul(ctx.mul(p.gam, p.rstd, "gam*rstd"), inner, "yt")
    return ctx.mul(yt, ctx.mask(y, p.slope, "tan mask"), "at")


def dbl_terms(ctx, z, qa, zt, ga1, p):
    """DblRedF::accum: ga1 * mk * zt [2]; qy = qa * mk [1], qy * xh [1]"""
    xh, y = _xh_y(ctx, z, p)
    mk = ctx.mask(y, p.slope, "dbl mask")
    gy = ctx.mul(ga1, mk, "gy")
    t0 = ctx.mul(gy, zt, "gy*zt")
    if qa is None:
        return xh, mk, gy, t0, None, None, None
    qy = ctx.mul(qa, mk, "qy")
    return xh, mk, gy, t0, qy, ctx.mul(qy, xh, "qy*xh"), qy


def dbl_fin_tree(ctx, s, sums, p, inv_m_total, m_local, raw_local=None):
    """DblFin / DblFinSync: s = the three (global) sums, sums = (s_gy, s_gyxh, s_zt, s_xhzt) global, raw_local = this rank's
    [_, s_qy, s_qyxh] (DblFinSync; DblFin uses s).  Returns (coef[5], dg, db)."""
    s_gy, s_gyxh, s_zt, s_xhzt = sums
    b, cc = ctx.mul(s_gyxh, inv_m_total, "b"), ctx.mul(s_xhzt, inv_m_total, "c")
    A = ctx.sub(ctx.mul(s[0], inv_m_total, "s0/m"),
                ctx.mul(ctx.mul(s_gy, inv_m_total, "sgy/m"), ctx.mul(s_zt, inv_m_total, "szt/m"), "mgy*mzt"), "A")
    bc = ctx.mul(b, cc, "b*c")
    k0 = ctx.sub(A, ctx.mul(ctx.mul(ctx.leaf(3.0), b, "3b"), cc, "3bc"), "A-3bc")
    k3, k4 = ctx.mul(s[1], inv_m_total, "k3"), ctx.mul(s[2], inv_m_total, "k4")
    loc = s if raw_local is None else raw_local
    dg = ctx.add(ctx.mul(ctx.mul(m_local, p.rstd, "m*invstd"), ctx.sub(A, bc, "A-bc"), "m/s(A-bc)"), loc[2], "dg")
    return (k0, cc, b, k3, k4), dg, loc[1]


def dbl_apply_tree(ctx, z, qa, zt, ga1, p, coef, s_gy, s_zt, inv_m):
    """DblApplyF::finish"""
    k0, k1, k2, k3, k4 = coef
    mgy, mzt = ctx.mul(s_gy, inv_m, "mgy"), ctx.mul(s_zt, inv_m, "mzt")
    xh, y = _xh_y(ctx, z, p)
    mk = ctx.mask(y, p.slope, "dbl apply mask")
    gy = ctx.mul(ga1, mk, "gy")
    r0 = ctx.add(ctx.add(ctx.mul(xh, k0, "xh*k0"), ctx.mul(k1, ctx.sub(gy, mgy, "gy-mgy"), "k1*()"), "r0a"),
                 ctx.mul(k2, ctx.sub(zt, mzt, "zt-mzt"), "k2*()"), "r0")
    out = ctx.mul(ctx.neg(ctx.mul(ctx.mul(p.gam, p.rstd, "gm*is"), p.rstd, "gm*is*is")), r0, "out")
    if qa is not None:
        q = ctx.sub(ctx.sub(ctx.mul(qa, mk, "qa*mk"), k3, "-k3"), ctx.mul(xh, k4, "xh*k4"), "q")
        out = ctx.add(out, ctx.mul(ctx.mul(p.gam, p.rstd, "gm*is"), q, "gm*is*q"), "out+q")
    return out


def inv_m_leaf(ctx, M):
    """1.f / (float)M: exact for a power of two, one rounding otherwise"""
    v = torch.tensor(1.0 / M, dtype=torch.float64)
    return ctx.leaf(v) if M & (M - 1) == 0 else ctx.leaf(v, U32 / M)


class Family:
    """every op of the BatchNorm family on one operand set, as trees: the references (fields .v) and, in bound mode, the
    bounds (.e).  W ranks of M rows each are simulated by passing the rows of one rank with the GLOBAL sums (sync=...)."""

    def __init__(self, ops, exact, M_total=None, rows=None, with_qa=True, y_exact=False, applies=True, dbl_apply=True,
                 strict_leaves=True):
        """applies = False: sums and the forward only (exact mode at an M that is no power of two, where 1 / M is rounded)"""
        o = ops
        ctx = self.ctx = Ctx(exact, y_exact, strict_leaves)
        sl = slice(None) if rows is None else rows
        z, ga, zt, qa = (ctx.leaf(o[k]) for k in ("z", "ga", "zt", "qa"))
        p = self.p = P(ctx, o["mean"], o["invstd"], o["gamma"], o["beta"], o["slope"])
        Mg = z.v.shape[0] if M_total is None else M_total
        self.M_total = Mg
        inv_m = inv_m_leaf(ctx, Mg)
        # ---- forward
        self.a, self.y_act = bn_act_tree(ctx, z, p)
        # ---- sums over the WHOLE batch (what an all-reduce of the rank sums gives, in any order)
        xh, y, mk, gy, gyxh = bwd_terms(ctx, z, ga, p)
        self.y, self.mk = y, mk
        self.s_gy, self.s_gyxh = ctx.colsum(gy, "s_gy"), ctx.colsum(gyxh, "s_gyxh")
        _, _, xhzt = tan_terms(ctx, z, zt, p)
        self.s_zt, self.s_xhzt = ctx.colsum(zt, "s_zt"), ctx.colsum(xhzt, "s_xhzt")
        self.colsum_ga = ctx.colsum(ga, "col_sum")
        self.sum_z, self.sum_zz = ctx.colsum(z, "sum z"), ctx.colsum(ctx.mul(z, z, "z*z"), "sum z^2")
        cutg = lambda t: EV(t.v[sl], t.e[sl])
        # one rank's share of the first backward's parameter gradients
        self.dgamma_local, self.dbeta_local = ctx.colsum(cutg(gyxh), "dgamma local"), ctx.colsum(cutg(gy), "dbeta local")
        if applies:
            self.gz = bwd_apply_tree(ctx, xh, gy, p, self.s_gy, self.s_gyxh, inv_m)
            self.at = tan_apply_tree(ctx, xh, y, zt, p, self.s_zt, self.s_xhzt, inv_m)
        # ---- double backward, with and without qa; the parameter gradients of the rows `sl` alone (one rank's share)
        self.dbl = {}
        for use_qa in ((True, False) if with_qa else (False,)):
            _, _, _, t0, t1, t2, _ = dbl_terms(ctx, z, qa if use_qa else None, zt, ga, p)
            zero = EV(torch.zeros_like(self.s_gy.v))
            s = [ctx.colsum(t0, "s_gyzt"), ctx.colsum(t1, "s_qy") if use_qa else zero, ctx.colsum(t2, "s_qyxh") if use_qa else zero]
            cut = lambda t: EV(t.v[sl], t.e[sl])
            loc = [None, ctx.colsum(cut(t1), "s_qy local") if use_qa else zero,
                   ctx.colsum(cut(t2), "s_qyxh local") if use_qa else zero]
            self.dbl[use_qa] = {"sums": s, "local": loc}
            if not applies:
                continue
            m_local = ctx.leaf(float(z.v[sl].shape[0]))
            coef, dg, db = dbl_fin_tree(ctx, s, (self.s_gy, self.s_gyxh, self.s_zt, self.s_xhzt), p, inv_m, m_local, loc)
            self.dbl[use_qa].update({"dg": dg, "db": db})
            if not dbl_apply:
                continue
            pz = dbl_apply_tree(ctx, z, qa if use_qa else None, zt, ga, p, coef, self.s_gy, self.s_zt, inv_m)
            self.dbl[use_qa]["pz"] = pz


# ------------------------------------------------------------------ operands
SLOPE_EXACT = 0.5


def exact_operands(M, C, seed):
    """Integers and powers of two inside bf16's 8 bits:  z = mean + d with d a non-zero integer in -4..4 and mean in -1..1
    (|z| <= 5, and z != 0 outside the planted elements), ga / zt / qa non-zero integers in -3..3, invstd in {1/2, 1}, |gamma| in
    {1, 2, 4}, beta a multiple of 1/2, slope 1/2.  Then xh, y, the mask, every product and every partial sum in any order are
    exact in fp32, and a = lrelu(y) (multiples of 1/4 up to 32) is exact in bf16.
    y == 0 is PLANTED: a channel with c % 4 == 0 gets beta = -d0 invstd gamma for a d0 of its own, and d = d0 in the rows with
    (r + c) % 16 == 0 and nowhere else; every other channel gets invstd = 1 and beta = an odd multiple of 1/2, where y cannot
    vanish."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    nz = lambda hi, shape: ri(1, hi, shape) * (ri(0, 1, shape) * 2 - 1)
    c = torch.arange(C)
    plant = (c % 4 == 0)
    mean = ri(-1, 1, (C,))
    invstd = torch.where(plant, 2.0 ** -ri(0, 1, (C,)), torch.ones(C, dtype=torch.float64))
    gamma = 2.0 ** ri(0, 2, (C,)) * (ri(0, 1, (C,)) * 2 - 1)
    d0 = nz(4, (C,))
    beta = torch.where(plant, -d0 * invstd * gamma, (ri(-4, 3, (C,)) + 0.5))
    # the values d may take in channel c: non-zero, not -mean (z != 0), not d0 in a planted channel; drawn through a table
    vals = torch.tensor([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    ok = (vals[None, :] != -mean[:, None]) & ~(plant[:, None] & (vals[None, :] == d0[:, None]))
    cnt = ok.sum(1)                                                   # 6 .. 8 per channel
    order = torch.argsort((~ok).int(), dim=1, stable=True)            # allowed values first
    pick = torch.randint(0, 840, (M, C), generator=gen) % cnt[None, :]
    d = vals[order[c[None, :].expand(M, C), pick]]
    here = plant[None, :] & ((torch.arange(M)[:, None] + c[None, :]) % 16 == 0)
    d = torch.where(here, d0[None, :].expand(M, C), d)
    return {"z": mean[None, :] + d, "ga": nz(3, (M, C)), "zt": nz(3, (M, C)), "qa": nz(3, (M, C)), "mean": mean, "invstd": invstd,
            "gamma": gamma, "beta": beta, "slope": SLOPE_EXACT, "planted": here}


def gauss_operands(M, C, seed, dtype, mean_from_z=True):
    """part B: Gaussian operands rounded to the storage type, arbitrary gamma / beta (fp32 numbers), slope 0.2; mean / invstd
    are the fp32 roundings of z's own statistics"""
    r = lambda t: t.float().to(dtype).double()
    z = r(gauss((M, C), seed) * 1.5 + 0.3)
    f32 = lambda t: t.float().double()
    mean = f32(z.mean(0)) if M > 1 else f32(gauss((C,), seed + 9) * 0.1)
    var = ((z - mean) ** 2).mean(0) if M > 1 else torch.ones(C, dtype=torch.float64)
    return {"z": z, "ga": r(gauss((M, C), seed + 1)), "zt": r(gauss((M, C), seed + 2)), "qa": r(gauss((M, C), seed + 3)),
            "mean": mean, "invstd": f32(torch.rsqrt(var + 1e-5)), "gamma": f32(1 + 0.1 * gauss((C,), seed + 4)),
            "beta": f32(0.1 * gauss((C,), seed + 5)), "slope": 0.2}


class Recorder:
    """stat_reduce of phase 1 of the rank simulation: keeps every local tensor, in call order"""

    def __init__(self):
        self.seen = []

    def __call__(self, t):
        self.seen.append(t.clone())


class Player:
    """stat_reduce of phase 2: writes the sum over the ranks of the tensors recorded at the same call index"""

    def __init__(self, recs):
        self.totals = [torch.stack(ts).sum(0) for ts in zip(*[r.seen for r in recs])]
        self.i = 0

    def __call__(self, t):
        t.copy_(self.totals[self.i])
        self.i += 1


def two_phase(ops_obj, W, fn, first=None, after=None):
    """One process, no process group: fn(k) runs one op on part k.  Phase 1 on every part with a stat_reduce that records the
    part's local tensors; phase 2 again on every part with a stat_reduce that writes the recorded totals; stat_world = W both
    times.  The local sums of one op do not depend on the reduced value, so phase 2 is the W-rank run.  `first` (a dict) tells
    an fn that changes buffers of its own (accumulated gradients, running statistics) which phase runs."""
    ops_obj.stat_world = W
    recs = []
    for k in range(W):
        rec = Recorder()
        ops_obj.stat_reduce = rec
        fn(k)
        recs.append(rec)
    if after is not None:
        after("phase 1")
    if first is not None:
        first["on"] = False
    outs = []
    for k in range(W):
        pl = Player(recs)
        ops_obj.stat_reduce = pl
        outs.append(fn(k))
        assert pl.i == len(pl.totals)
    ops_obj.stat_reduce, ops_obj.stat_world = None, 1
    if after is not None:
        after("phase 2")
    return outs


def rank_rows(M_rank, W, k):
    return slice(k * M_rank, (k + 1) * M_rank)


# ------------------------------------------------------------------ conditions (part A), on the reference alone
def frac_zero(t):
    return float((t == 0).double().mean())


def tensor_condition(t, what):
    """at most 10 % zeros; at least 50 distinct values -- or, where the operand ranges cannot give 50: an eighth of the elements
    of a tensor of fewer than 400, and 4 per channel (a channel's elements take 9 values at most, the 8 of d and the planted
    one, and the channels' sets overlap)"""
    assert frac_zero(t) <= 0.10, "%s: %.1f %% zeros" % (what, 100 * frac_zero(t))
    need = min(50, t.numel() // 8, 4 * t.shape[-1])
    assert int(torch.unique(t).numel()) >= need, "%s: %d distinct values < %d" % (what, int(torch.unique(t).numel()), need)


def vector_condition(v, what):
    assert frac_zero(v) <= 0.10, "%s: %.1f %% zero entries" % (what, 100 * frac_zero(v))
    assert v.numel() == 1 or int(torch.unique(v).numel()) > 1, what + ": all entries equal"


def mask_condition(y, what):
    f = float((y > 0).double().mean())
    assert 0.2 <= f <= 0.8, "%s: the mask takes %.1f %% of the elements" % (what, 100 * f)


def storable(t, dtype, what):
    assert torch.equal(t.float().to(dtype).double(), t), "%s does not survive a round trip through %s" % (what, dtype)


def exact_level(M):
    """what of a case is EXACT in fp32: the sums and the forward always; gz / at and the double backward's parameter gradients
    when 1 / M is (M a power of two); pz when moreover M <= 64 (its coefficients carry 1 / M^2: at M = 1024 the products of
    two means need more than 24 bits).  The rest of a case is held to the bound of the same trees."""
    pow2 = M & (M - 1) == 0
    return pow2, pow2 and M <= 64


def exact_conditions(ops, fam, dtype, what, pow2):
    """every condition of part A on one case (fam = Family(ops, exact=True): the tree nodes were asserted while it was built)"""
    for k in ("z", "ga", "zt", "qa"):
        storable(ops[k], dtype, what + " " + k)
    storable(fam.a.v, dtype, what + " a")
    assert int(ops["planted"].sum()) >= 1 and bool((fam.y.v[ops["planted"]] == 0).all()), what + ": no planted y == 0"
    assert bool((fam.mk.v[fam.y.v == 0] == ops["slope"]).all())
    mask_condition(fam.y.v, what)
    outs = [("a", fam.a.v)]
    if pow2:
        outs += [("gz", fam.gz.v), ("at", fam.at.v)]
    if "pz" in fam.dbl[True]:
        outs += [("pz+qa", fam.dbl[True]["pz"].v), ("pz", fam.dbl[False]["pz"].v)]
    for name, t in outs:
        tensor_condition(t, what + " " + name)
    vecs = [("s_gy", fam.s_gy.v), ("s_gyxh", fam.s_gyxh.v), ("s_zt", fam.s_zt.v), ("s_xhzt", fam.s_xhzt.v),
            ("sum z", fam.sum_z.v), ("sum z^2", fam.sum_zz.v), ("col_sum", fam.colsum_ga.v)]
    if pow2:
        vecs += [("dbl dgamma+qa", fam.dbl[True]["dg"].v), ("dbl dbeta+qa", fam.dbl[True]["db"].v), ("dbl dgamma", fam.dbl[False]["dg"].v)]
    if ops["z"].shape[1] >= 20:
        for name, v in vecs:
            vector_condition(v, what + " " + name)
    else:                                     # a vector of fewer than 10 entries: 10 % of them is no entry at all
        for name, v in vecs:
            assert int((v == 0).sum()) <= v.numel() // 10 and int(torch.unique(v).numel()) > 1, what + " " + name


# ------------------------------------------------------------------ statistics
def stats_ref(z, M_total, eps, momentum, rm, rv, E_s=None, E_ss=None):
    """StatsFinalizeFin / bn_finalize_kernel on the fp64 sums of z (the rows of every rank): mean, invstd, running statistics
    and their bounds.  eps and momentum are the fp32 numbers the kernels receive.  Roundings, read off the finisher:
        mean    fl32(s / m), the quotient formed in fp64                                        1 unit of |mean|
        var     fl32(max(ss / m - mu^2, 0)), the subtraction in fp64                            1 unit of var
        invstd  rsqrtf(var + eps): the sum [1] and v_rsq_f32 at 1 ulp [2]                        d/dx rsqrt = -invstd / 2x
        unb     var * (m / fmaxf(m - 1, 1)): the quotient at 1 ulp [2], the product [1]
        running (1 - momentum) [1] * r [1] + momentum * x [1], the sum [1]                       4 units of the terms
    E_s / E_ss: the error of the fp32 column sums (default: any order over the rows of z; 0 for integer z)."""
    s, ss = z.sum(0), (z * z).sum(0)
    M = z.shape[0]
    g = (M - 1) * U32 / (1 - (M - 1) * U32)
    E_s = g * z.abs().sum(0) if E_s is None else E_s
    E_ss = (g + 2 * U32) * (z * z).sum(0) if E_ss is None else E_ss              # (+ the product's own rounding)
    m = float(M_total)
    mu, var = s / m, torch.clamp(ss / m - (s / m) ** 2, min=0.0)
    e_mu = E_s / m + U32 * mu.abs()
    e_var_sum = E_ss / m + 2 * mu.abs() * E_s / m + (E_s / m) ** 2                 # what the fp32 SUMS cost the variance
    e_var = e_var_sum + U32 * var
    x = var + eps
    e_x = e_var + U32 * x
    inv = torch.rsqrt(x)
    e_inv = 0.5 * inv / (x - e_x).clamp_min(1e-300) * e_x + 2 * U32 * inv
    k = m / max(m - 1.0, 1.0)
    unb = var * k
    e_unb = e_var * k + 3 * U32 * unb
    out = {"mean": mu, "e_mean": e_mu, "var": var, "e_var_sum": e_var_sum, "invstd": inv, "e_invstd": e_inv}
    if rm is not None:
        out["rm"] = (1 - momentum) * rm + momentum * mu
        out["e_rm"] = 4 * U32 * ((1 - momentum) * rm.abs() + momentum * mu.abs()) + momentum * e_mu
        out["rv"] = (1 - momentum) * rv + momentum * unb
        out["e_rv"] = 4 * U32 * ((1 - momentum) * rv.abs() + momentum * unb.abs()) + momentum * e_unb
    return out


def latent_ref(u, z, split):
    """latent_prep in fp64 on the whole batch, (v - mean) / std with the unbiased std of torch.std, and its bound.
    split = False: latent_prep_kernel / latent_prep_big_kernel (two passes: mean, then sum (v - mean)^2).
    split = True:  rg_latent_stats + rg_latent_apply on all-reduced sums (one pass: var = max(ss - nt mu^2, 0) / (nt - 1)).
    Roundings: v = u + z [1]; the column sums in any order [(n - 1) units of sum |t|]; a division or a square root at 1 ulp
    [2 units each: HIP's documented maximum]; every other operation [1]."""
    v = u + z
    n = v.shape[0]
    g = (n - 1) * U32 / (1 - (n - 1) * U32)
    e_v = U32 * v.abs()
    mu = v.mean(0)
    e_mu = (e_v.sum(0) + g * (v.abs() + e_v).sum(0)) / n + 2 * U32 * mu.abs()
    d = v - mu
    e_d = e_v + e_mu + U32 * d.abs()
    if split:
        sq, e_sq = v * v, 2 * v.abs() * e_v + e_v ** 2 + U32 * v * v
        ss = sq.sum(0)
        e_ss = e_sq.sum(0) + g * (sq + e_sq).sum(0)
        nm2 = n * mu * mu
        e_nm2 = n * (2 * mu.abs() * e_mu + e_mu ** 2) + 2 * U32 * nm2
        q = (ss - nm2).clamp_min(0.0)
        e_q = e_ss + e_nm2 + U32 * q
    else:
        sq, e_sq = d * d, 2 * d.abs() * e_d + e_d ** 2 + U32 * d * d
        q = sq.sum(0)
        e_q = e_sq.sum(0) + g * (sq + e_sq).sum(0)
    var = q / (n - 1)
    e_var = e_q / (n - 1) + 2 * U32 * var
    sd = var.sqrt()
    e_sd = e_var / (2 * (var - e_var).clamp_min(1e-300).sqrt()) + 2 * U32 * sd
    ref = d / sd
    return ref, e_d / (sd - e_sd) + d.abs() * e_sd / (sd * (sd - e_sd)) + 2 * U32 * ref.abs() + 2.0 ** -140


# ------------------------------------------------------------------ partial rows (part D)
def partial_rows(z, G):
    """[G][2][C] column sums of z's rows cut into G consecutive tiles (sizes as even as M allows; a tile may be empty when
    G > M): what a conv epilogue leaves"""
    M, C = z.shape
    edges = [(g * M) // G for g in range(G + 1)]
    out = torch.zeros((G, 2, C), dtype=torch.float64)
    for g in range(G):
        t = z[edges[g]:edges[g + 1]]
        out[g, 0], out[g, 1] = t.sum(0), (t * t).sum(0)
    return out


def partial_rows_g2(z2, G, nblk):
    """two halves of z2 [2 M][C], G partial rows each, laid out [nblk][2 halves][G / nblk] (rg_bn_forward_g2)"""
    M = z2.shape[0] // 2
    assert G % nblk == 0
    Gb = G // nblk
    halves = [partial_rows(z2[h * M:(h + 1) * M], G) for h in range(2)]
    out = torch.zeros((2 * G, 2, z2.shape[1]), dtype=torch.float64)
    for b in range(nblk):
        for h in range(2):
            out[(b * 2 + h) * Gb:(b * 2 + h + 1) * Gb] = halves[h][b * Gb:(b + 1) * Gb]
    return out


def ints_z(M, C, seed, lo=-3, hi=3):
    gen = torch.Generator().manual_seed(seed)
    off = torch.randint(-1, 2, (C,), generator=gen).double()
    return torch.randint(lo, hi + 1, (M, C), generator=gen).double() + off


def partial_condition(part, z, M):
    """(D): the partial rows are fp32 numbers whose sums in any order are exact, M is a power of two, so mean is a dyadic
    rational that fp32 holds: it must come out bit-equal"""
    assert M & (M - 1) == 0 and z.shape[0] == M
    assert torch.equal(part.float().double(), part)
    assert float((z * z).sum(0).max()) < 2 ** 24 and torch.equal(part.sum(0)[0], z.sum(0)) and torch.equal(part.sum(0)[1], (z * z).sum(0))
    mean = z.sum(0) / M
    assert torch.equal(mean.float().double(), mean)
    vector_condition(mean, "mean of the partial rows") if z.shape[1] >= 20 else None
    assert int(torch.unique(mean).numel()) > 1
