"""The betaVAE-training and FID kernels, op by op, against fp64 -- the entry points rna_gan_amd/vae_train.py and
rna_gan_amd/inception.py call through the C ABI directly (lib.rg_*), which no HipOps-level test drives.

Three kinds of check (the pattern of tests/test_ops_exact_gpu.py):
(E) EXACT.  Operands are integers in {-3..3}, affine factors powers of two, shifts small integers: every partial sum in any
    order, through split-K slabs too, is an integer (or a multiple of 0.5) below 2^24, so the result must equal the fp64
    product cast to fp32.  S = sum |a||b| |scale| + |shift| <= 2^24 is a CONDITION, asserted on the reference before comparing
    (here and, without a kernel, in tests/test_vae_fid_refs_cpu.py).
(B) BOUND.  Random operands, reference = fp64 product of the operands as rounded to the storage type, element-wise
    |got - ref| <= u |ref| + K 2^-24 (1 + u) S + 2^-25 with u = 2^-24 (fp32 outputs), S = sum |a||b| in fp64, K the contraction
    length + 1 per epilogue factor; only at K <= 1025 (above, the bound is vacuous and (E) alone decides).
(S) SENTINEL.  Outputs live inside a larger allocation pre-filled with one finite bit pattern: what the contract leaves
    untouched must keep it bit for bit, what it zero-fills must be +0.0.  Operands live inside a larger allocation whose
    remainder is NaN: a row or column read past the operand shows up as a non-finite output.  Those reads stay inside the
    allocation, so nothing can fault.

Every worst |err| / bound of a (B) case is printed as "RATIO <op> <case> <value>" (profiles/vae_fid_op_errors.txt records them;
the gates are derived, the file only documents the headroom).  bf16 build only (VaeRuntime is), except the packed linear cases.
"""
import numpy as np
import pytest
import torch

import vae_fid_refs as R
from both_builds import fp16_twin
from guarded import DEV, SBITS, Guarded, _assert_sentinel, _out
from vae_fid_refs import SENTINEL, U32, bits, ceil64

pytestmark = pytest.mark.gpu
NAN = float("nan")


class _Env:
    def __init__(self, h16=torch.bfloat16):
        from rna_gan_amd import _abi
        from rna_gan_amd.ops_hip import HipOps
        self.abi = _abi
        self.ops = HipOps(h16, DEV)
        self.lib = self.ops.lib if h16 != torch.bfloat16 else _abi.load()
        self.h16 = h16

    @property
    def stream(self):
        return self.ops.stream

    def ok(self, rc, what):
        self.abi.check(rc, what)
        torch.cuda.synchronize()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def _assert_pos_zero(t, what):
    assert bool((bits(t) == 0).all()), "%s: %d elements that must be +0.0 are not" % (what, int((bits(t) != 0).sum()))


def _exact(got, ref, what):
    got, ref = got.detach().cpu().float(), ref.detach().cpu().float()
    assert torch.isfinite(got).all(), what + ": non-finite output (a guard region was read?)"
    bad = got != ref                                                      # by value: -0.0 == +0.0
    assert not bool(bad.any()), "%s: %d of %d outputs differ, first at %s" % (what, int(bad.sum()), bad.numel(),
                                                                            bad.nonzero()[:4].tolist())


def _bound_check(got, ref, S, K, op, case):
    """tests/test_ops_exact_gpu.py::_bound_check with u = 2^-24 (an fp32 result); nothing in it is measured"""
    assert K <= 1025, "the bound is vacuous above K = 1024 (+ 1 where an epilogue factor adds a rounding)"
    got, ref, S = got.detach().cpu().double(), ref.double(), S.double()
    assert torch.isfinite(got).all(), "%s %s: non-finite output (a guard region was read?)" % (op, case)
    bnd = U32 * ref.abs() + K * 2.0 ** -24 * (1 + U32) * S + 2.0 ** -25
    ratio = float(((got - ref).abs() / bnd).max())
    print("RATIO %s %s %.4f" % (op, case, ratio))
    bad = (got - ref).abs() > bnd
    assert not bool(bad.any()), "%s %s: %d of %d outputs outside the worst-case bound (worst ratio %.2f), first at %s" % (
        op, case, int(bad.sum()), bad.numel(), ratio, bad.nonzero()[:4].tolist())


def _act64(ref, S, slope):
    """the activation on the fp64 reference: lrelu is 1-Lipschitz, so the pre-activation bound carries over; a slope other than
    0 / 1 is one more rounded factor (the caller adds 1 to K)"""
    s32 = float(np.float32(slope))
    return torch.where(ref > 0, ref, ref * s32), S


# ================================================================== rg_gemm_nt_bf16
# (name, M, K_pad, Nout, ldy).  The plan a launch takes, quoted from launch_gather2 / gather_split of rg_mfma.hip for
# EPI_LINEAR, MODE_PLAIN (fp32 output: neither the 8-wave nor the 256 x 256 tile applies):
#     narrow (256 x 64 tile)   Nout <= 64
#     stream (64 x 128 tile)   M <= 64 and Nout > 64
#     t128   (128 x 128 tile)  otherwise
#     split-K                  tiles < 512 and K_pad / 64 >= 16, s = min(ceil(512 / tiles), 16, K_pad / 512) > 1, and only when
#                              Nout % 8 == 0, ldy % 4 == 0 and the workspace holds s * M * ldy floats
# rg_gemm_nt_bf16_workspace_bytes returns s * M * Nout * 4 + 256 when the plan splits and 256 when it does not: "> 256" is the
# split, "== 256" is no split.
GEMM_CASES = [
    ("stream", 5, 64, 72, 72),
    ("stream+split", 40, 1024, 136, 136),
    ("narrow-ragged-rows", 300, 128, 24, 24),
    ("t128-ragged-both", 130, 128, 200, 200),
    ("t128-wgrad-form", 520, 64, 264, 264),
    ("t128-ragged70", 130, 64, 70, 70),
    ("stream-odd-pitch515", 40, 64, 515, 515),
    ("stream-pitch774", 40, 64, 774, 774),
    ("stream-pad70in128", 5, 64, 70, 128),
    ("narrow-pad10in12", 5, 64, 10, 12),
    ("stream-nosplit-ws-from-Nout", 40, 1024, 136, 192),
]
LINEAR_EXACT_SHAPES = [(37, 27, 32), (70, 48, 64), (129, 5, 7), (5, 4100, 70), (16, 200, 136), (6, 50, 24), (70, 100, 72)]


def _plan(M, Kp, Nout, ldy):
    tile = "narrow" if Nout <= 64 else "stream" if M <= 64 else "t128"
    bn, bm = (64, 256) if Nout <= 64 else (128, 128)                      # gather_split's own tile count
    tiles, nkt = -(-M // bm) * -(-Nout // bn), Kp // 64
    s = 1 if (tiles >= 512 or nkt < 16) else max(1, min(-(-512 // tiles), 16, nkt // 8))
    return tile, s


def gemm_operands_int(M, Kp, Nout):
    return R.ints((M, Kp), 1000 + M), R.ints((Nout, Kp), 2000 + Nout)


def _gemm_launch(env, a, b, scale, shift, M, Kp, Nout, ldy, slope):
    """y inside a sentinel allocation; the workspace is exactly what the query says (HipOps._ws may hand out a larger, cached
    buffer: the byte count passed is the query's, so that a split that needs more than the query promises cannot happen)"""
    y = _out((M, ldy))
    q = env.lib.rg_gemm_nt_bf16_workspace_bytes(M, Kp, Nout)
    ws = env.ops._ws(q)
    env.ok(env.lib.rg_gemm_nt_bf16(_ptr(a), _ptr(b), _ptr(scale), _ptr(shift), _ptr(y.t), ldy, M, Kp, Nout, float(slope),
                                   _ptr(ws), q, env.stream), "rg_gemm_nt_bf16")
    return y, q


def _gemm_sentinels(y, M, Nout, ldy, what):
    """the header's contract: columns Nout .. min(roundup8(Nout), ldy) - 1 are +0.0, the rest of the row and everything around
    the matrix is untouched"""
    z1 = min((Nout + 7) // 8 * 8, ldy)
    if z1 > Nout:
        _assert_pos_zero(y.t[:, Nout:z1], what + " pad columns %d..%d" % (Nout, z1 - 1))
    if ldy > z1:
        _assert_sentinel(y.t[:, z1:], what + " columns %d..%d" % (z1, ldy - 1))
    assert y.surroundings_keep(SBITS), what + ": wrote outside y"


EPILOGUES = [("plain", False, False, 1.0), ("affine-lrelu", True, True, 0.01), ("shift-relu", False, True, 0.0),
             ("scale", True, False, 1.0), ("affine-relu", True, True, 0.0)]


def _guard_rows(Kp):
    return 256 * Kp                                                        # one 256-row tile past the operand's last row


@pytest.mark.parametrize("name,M,Kp,Nout,ldy", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_nt_bf16_exact_integers(name, M, Kp, Nout, ldy):
    """(E) + (S) on hand-built bf16 operands ([M][K_pad] and [Nout][K_pad] exact, NaN after the last row of each), every
    epilogue; the id names the plan, the assertions below hold the launch to it."""
    env = _Env()
    tile, s = _plan(M, Kp, Nout, ldy)
    assert name.startswith(tile)
    q = env.lib.rg_gemm_nt_bf16_workspace_bytes(M, Kp, Nout)
    if "+split" in name:
        assert s > 1 and q > 256 and q == s * M * Nout * 4 + 256 and Nout % 8 == 0 and ldy % 4 == 0 and q - 256 >= s * M * ldy * 4
    elif "nosplit-ws-from-Nout" in name:
        assert s > 1 and q > 256 and q - 256 < s * M * ldy * 4            # sized from Nout, needed for ldy: falls back to no split
    else:
        assert s == 1 and q == 256
    a64, b64 = gemm_operands_int(M, Kp, Nout)
    a = Guarded(a64.to(torch.bfloat16), NAN, after=_guard_rows(Kp))
    b = Guarded(b64.to(torch.bfloat16), NAN, after=_guard_rows(Kp))
    sc64, sh64 = R.pow2_affine(Nout, 7)
    sc = Guarded(sc64.float(), NAN)
    sh = Guarded(sh64.float(), NAN)
    for ename, use_sc, use_sh, slope in EPILOGUES:
        ref, S = R.gemm_ref(a64, b64, sc64 if use_sc else None, sh64 if use_sh else None)
        R.exact_condition(ref, S, name)
        y, _ = _gemm_launch(env, a.t, b.t, sc.t if use_sc else None, sh.t if use_sh else None, M, Kp, Nout, ldy, slope)
        what = "gemm_nt_bf16[%s, %s]" % (name, ename)
        _exact(y.t[:, :Nout], R.lrelu32(ref.float(), slope), what)
        if slope == 0.0:
            assert float(ref.min()) < 0 < float(ref.max())                # outputs straddle zero
        _gemm_sentinels(y, M, Nout, ldy, what)


@pytest.mark.parametrize("name,M,Kp,Nout,ldy", [c for c in GEMM_CASES], ids=[c[0] for c in GEMM_CASES])
def test_gemm_nt_bf16_kernel_built_operands_bound(name, M, Kp, Nout, ldy):
    """(B) + (S) on operands the library's own kernels build, the way vae_train.py does: A from rg_cast_pad (K = K_pad - 5: five
    zero pad columns) or, for the weight-gradient form, both operands from rg_transpose_pack_bf16 (K = batch 40, padded to 64);
    B from HipOps.pack_linear (rows padded to a multiple of 128).  Each is copied into a NaN-guarded allocation."""
    env = _Env()
    lib = env.lib
    if "wgrad" in name:
        batch = 40
        gy, x = R.gauss((batch, M), 31), R.gauss((batch, Nout), 32)
        a_dev = torch.full((M, Kp), NAN, dtype=torch.bfloat16, device=DEV)
        b_dev = torch.full((Nout, Kp), NAN, dtype=torch.bfloat16, device=DEV)
        env.ok(lib.rg_transpose_pack_bf16(_ptr(_dev(gy)), _ptr(a_dev), batch, M, Kp, M, env.stream), "rg_transpose_pack_bf16")
        env.ok(lib.rg_transpose_pack_bf16(_ptr(_dev(x)), _ptr(b_dev), batch, Nout, Kp, Nout, env.stream), "rg_transpose_pack_bf16")
        a64, b64 = gy.float().t().bfloat16().double(), x.float().t().bfloat16().double()
    else:
        K = Kp - 5
        xa, w = R.gauss((M, K), 33), R.gauss((Nout, K), 34, (1.0 / K) ** 0.5)
        a_dev = torch.full((M, Kp), NAN, dtype=torch.bfloat16, device=DEV)
        env.ok(lib.rg_cast_pad(_ptr(_dev(xa)), _ptr(a_dev), M, K, Kp, env.abi.RG_BF16, env.stream), "rg_cast_pad")
        b_dev = env.ops.pack_linear(_dev(w))
        torch.cuda.synchronize()
        assert b_dev.shape == ((Nout + 127) // 128 * 128, Kp)
        a64, b64 = xa.float().bfloat16().double(), w.float().bfloat16().double()
    # the operand images are what the reference assumes: rounded values, exact zeros in the pads
    Kr = a64.shape[1]
    assert torch.equal(a_dev[:, :Kr].cpu().double(), a64) and bool((bits(a_dev[:, Kr:].float()) == 0).all())
    assert torch.equal(b_dev[:Nout, :Kr].cpu().double(), b64) and bool((b_dev[:Nout, Kr:].float() == 0).all())
    a = Guarded(a_dev, NAN, after=_guard_rows(Kp))
    b = Guarded(b_dev, NAN, after=_guard_rows(Kp))
    sc64, sh64 = 1 + 0.1 * R.gauss((Nout,), 35), 0.1 * R.gauss((Nout,), 36)
    sc64, sh64 = sc64.float().double(), sh64.float().double()
    sc, sh = Guarded(sc64.float(), NAN), Guarded(sh64.float(), NAN)
    ran = 0
    for ename, use_sc, use_sh, slope in EPILOGUES:
        Kb = Kp + int(use_sc) + int(use_sh) + int(slope not in (0.0, 1.0))
        if Kb > 1025:
            continue                                                       # (the K_pad = 1024 cases: plain and one-factor epilogues)
        ref, S = R.gemm_ref(a64, b64, sc64 if use_sc else None, sh64 if use_sh else None)
        ref, S = _act64(ref, S, slope)
        y, _ = _gemm_launch(env, a.t, b.t, sc.t if use_sc else None, sh.t if use_sh else None, M, Kp, Nout, ldy, slope)
        _bound_check(y.t[:, :Nout], ref, S, Kb, "rg_gemm_nt_bf16", "%s/%s" % (name, ename))
        _gemm_sentinels(y, M, Nout, ldy, "gemm_nt_bf16[%s, %s]" % (name, ename))
        ran += 1
    assert ran >= 2


# ================================================================== rg_linear_affine_act, fp32 generic path
def _linear_generic(env, x_ptr, ldx, w, scale, shift, y_ptr, ldy, M, K, Nout, slope, ws, ws_bytes):
    env.ok(env.lib.rg_linear_affine_act(x_ptr, ldx, _ptr(w), 0, _ptr(scale), _ptr(shift), y_ptr, ldy, M, K, Nout, float(slope),
                                        env.abi.ALGO_GENERIC, _ptr(ws), ws_bytes, env.stream), "rg_linear_affine_act")


SLICES = [(37, 27, 27, 0, 32, 32, 0), (70, 48, 288, 64, 64, 256, 64), (129, 5, 5, 0, 7, 9, 0)]     # M, K, ldx, c0, Nout, ldy, d0


@pytest.mark.parametrize("M,K,ldx,c0,Nout,ldy,d0", SLICES)
def test_linear_generic_channel_slices(M, K, ldx, c0, Nout, ldy, d0):
    """The strided forms Inception uses (ws = NULL, slope 0): x is columns c0..c0+K of a [M][ldx] buffer whose other columns
    are NaN, y is columns d0..d0+Nout of a [M][ldy] sentinel buffer.  (E) with outputs straddling zero, (B) on Gaussians, (S):
    every other column of y untouched."""
    env = _Env()
    for kind in ("E", "B"):
        if kind == "E":
            x64, w64 = R.ints((M, K), 21), R.ints((Nout, K), 22)
            sc64, sh64 = R.pow2_affine(Nout, 7)
        else:
            x64, w64 = R.gauss((M, K), 23).float().double(), R.gauss((Nout, K), 24, (1.0 / K) ** 0.5).float().double()
            sc64, sh64 = (1 + 0.1 * R.gauss((Nout,), 25)).float().double(), (0.1 * R.gauss((Nout,), 26)).float().double()
        xbuf = torch.full((M, ldx), NAN, dtype=torch.float32)
        xbuf[:, c0:c0 + K] = x64.float()
        xg = Guarded(xbuf, NAN)
        wg, sc, sh = Guarded(w64.float(), NAN), Guarded(sc64.float(), NAN), Guarded(sh64.float(), NAN)
        y = _out((M, ldy))
        _linear_generic(env, xg.t.data_ptr() + 4 * c0, ldx, wg.t, sc.t, sh.t, y.t.data_ptr() + 4 * d0, ldy, M, K, Nout, 0.0, None, 0)
        ref, S = R.gemm_ref(x64, w64, sc64, sh64)
        what = "linear_affine_act[slice %d x %d x %d, %s]" % (M, K, Nout, kind)
        got = y.t[:, d0:d0 + Nout]
        if kind == "E":
            R.exact_condition(ref, S, what)
            assert float(ref.min()) < 0 < float(ref.max())
            _exact(got, R.lrelu32(ref.float(), 0.0), what)               # by value: -0.0 (negative * 0) equals 0
        else:
            _bound_check(got, *_act64(ref, S, 0.0), K + 2, "rg_linear_affine_act", "slice%dx%dx%d" % (M, K, Nout))
        if d0:
            _assert_sentinel(y.t[:, :d0], what + " columns below the slice")
        if d0 + Nout < ldy:
            _assert_sentinel(y.t[:, d0 + Nout:], what + " columns above the slice")
        assert y.surroundings_keep(SBITS), what + ": wrote outside y"


def test_linear_generic_split_k_exact_with_and_without_workspace():
    """The fp32 split-K plan (M <= 128, K >= 4096): (M = 5, K = 4100, Nout = 70) once with the workspace the query asks for
    (> 0: the plan splits) and once with none (one launch over the whole K).  (E) on both, so both equal the reference bit for
    bit and hence each other.  Every epilogue, slope 0 included."""
    env = _Env()
    M, K, Nout = 5, 4100, 70
    q = env.lib.rg_linear_workspace_bytes(M, K, Nout, env.abi.ALGO_GENERIC)
    assert q > 0 and q % (M * Nout * 4) == 0 and q // (M * Nout * 4) >= 2
    assert env.lib.rg_linear_workspace_bytes(M, 4095, Nout, env.abi.ALGO_GENERIC) == 0      # below the threshold: no split
    x64, w64 = R.ints((M, K), 21), R.ints((Nout, K), 22)
    sc64, sh64 = R.pow2_affine(Nout, 7)
    xg, wg = Guarded(x64.float(), NAN, after=64 * K), Guarded(w64.float(), NAN, after=64 * K)
    sc, sh = Guarded(sc64.float(), NAN), Guarded(sh64.float(), NAN)
    ws = Guarded(torch.full((q // 4,), SENTINEL, dtype=torch.float32), SENTINEL)
    for ename, use_sc, use_sh, slope in EPILOGUES:
        ref, S = R.gemm_ref(x64, w64, sc64 if use_sc else None, sh64 if use_sh else None)
        R.exact_condition(ref, S, "linear split-K")
        want = R.lrelu32(ref.float(), slope)
        for with_ws in (True, False):
            y = _out((M, Nout))
            _linear_generic(env, _ptr(xg.t), K, wg.t, sc.t if use_sc else None, sh.t if use_sh else None, _ptr(y.t), Nout, M, K,
                            Nout, slope, ws.t if with_ws else None, q if with_ws else 0)
            what = "linear_affine_act[split-K %s, %s]" % ("ws" if with_ws else "no ws", ename)
            _exact(y.t, want, what)
            assert y.surroundings_keep(SBITS) and ws.surroundings_keep(SBITS), what + ": wrote outside y / the workspace"
    assert not bool((bits(ws.t) == SBITS).all())                           # the split launches did use the slabs


@pytest.mark.parametrize("M,K,Nout", [(5, 1024, 70), (70, 1000, 72), (6, 50, 24)])
def test_linear_generic_unsplit_bound(M, K, Nout):
    """(B) for the unsplit fp32 kernel at K <= 1024 (K + 2 epilogue roundings would pass the guard at 1024: that shape runs
    without scale)."""
    env = _Env()
    assert env.lib.rg_linear_workspace_bytes(M, K, Nout, env.abi.ALGO_GENERIC) == 0
    x64, w64 = R.gauss((M, K), 41).float().double(), R.gauss((Nout, K), 42, (1.0 / K) ** 0.5).float().double()
    sc64, sh64 = (1 + 0.1 * R.gauss((Nout,), 43)).float().double(), (0.1 * R.gauss((Nout,), 44)).float().double()
    use_sc = K + 3 <= 1025
    xg, wg = Guarded(x64.float(), NAN, after=64 * K), Guarded(w64.float(), NAN, after=64 * K)
    sc, sh = Guarded(sc64.float(), NAN), Guarded(sh64.float(), NAN)
    for slope in (0.01, 0.0) if use_sc else (0.0,):
        y = _out((M, Nout))
        _linear_generic(env, _ptr(xg.t), K, wg.t, sc.t if use_sc else None, sh.t, _ptr(y.t), Nout, M, K, Nout, slope, None, 0)
        ref, S = R.gemm_ref(x64, w64, sc64 if use_sc else None, sh64)
        _bound_check(y.t, *_act64(ref, S, slope), K + 1 + int(use_sc) + int(slope == 0.01), "rg_linear_affine_act",
                     "generic%dx%dx%d/slope%g" % (M, K, Nout, slope))
        assert y.surroundings_keep(SBITS)


@fp16_twin
@pytest.mark.parametrize("M,K,Nout,mfma", [(16, 200, 136, True), (6, 50, 24, True), (70, 100, 72, True), (6, 50, 70, False),
                                           (5, 200, 10, False)])
def test_linear_packed_auto(M, K, Nout, mfma, h16=torch.bfloat16):
    """wp from HipOps.pack_linear, ALGO_AUTO: Nout % 8 == 0 takes the matrix-core kernel (16-bit operands), Nout % 8 != 0 falls
    back to the fp32 generic kernel -- told apart by WHICH reference the result is held to: the MFMA result must be within (B) of
    the product of the operands rounded to the storage type, the fallback within (B) of the product of the fp32 operands (the
    two references differ by far more than either bound); (E) on both.  Both builds."""
    env = _Env(h16)
    assert (Nout % 8 == 0) == mfma
    algo = env.abi.ALGO_AUTO
    q = env.lib.rg_linear_workspace_bytes(M, K, Nout, algo)
    assert q >= M * ceil64(K) * 2
    for kind in ("E", "B"):
        if kind == "E":
            x64, w64 = R.ints((M, K), 21), R.ints((Nout, K), 22)
            sc64, sh64 = R.pow2_affine(Nout, 7)
        else:
            x64, w64 = R.gauss((M, K), 51).float().double(), R.gauss((Nout, K), 52, (1.0 / K) ** 0.5).float().double()
            sc64, sh64 = (1 + 0.1 * R.gauss((Nout,), 53)).float().double(), (0.1 * R.gauss((Nout,), 54)).float().double()
        x, w, sc, sh = _dev(x64), _dev(w64), _dev(sc64), _dev(sh64)
        wp = env.ops.pack_linear(w)
        ws = env.ops._ws(q)
        y = _out((M, Nout))
        env.ok(env.lib.rg_linear_affine_act(_ptr(x), K, _ptr(w), _ptr(wp), _ptr(sc), _ptr(sh), _ptr(y.t), Nout, M, K, Nout, 0.01,
                                            algo, _ptr(ws), q, env.stream), "rg_linear_affine_act")
        what = "linear_affine_act[packed %d x %d x %d, %s, %s]" % (M, K, Nout, kind, "mfma" if mfma else "generic fallback")
        if kind == "E":
            ref, S = R.gemm_ref(x64, w64, sc64, sh64)
            R.exact_condition(ref, S, what)
            _exact(y.t, R.lrelu32(ref.float(), 0.01), what)
        else:
            xr, wr = (x64.float().to(h16).double(), w64.float().to(h16).double()) if mfma else (x64, w64)
            ref, S = R.gemm_ref(xr, wr, sc64, sh64)
            Kc = ceil64(K) if mfma else K
            _bound_check(y.t, *_act64(ref, S, 0.01), Kc + 3, "rg_linear_affine_act",
                         "packed%dx%dx%d/%s" % (M, K, Nout, "bf16" if h16 == torch.bfloat16 else "fp16"))
            # a condition on the references alone: no result can be inside the bound of BOTH, so the check above tells the kernels apart
            xo, wo = (x64, w64) if mfma else (x64.float().to(h16).double(), w64.float().to(h16).double())
            other, _ = _act64(*R.gemm_ref(xo, wo, sc64, sh64), 0.01)
            ref_a, S_a = _act64(ref, S, 0.01)
            bnd = U32 * ref_a.abs() + (Kc + 3) * U32 * (1 + U32) * S_a + 2.0 ** -25
            assert bool(((other - ref_a).abs() > 2 * bnd).any()), what + ": the two references are too close to tell the kernels apart"
        assert y.surroundings_keep(SBITS), what + ": wrote outside y"


# ================================================================== transposes
TSHAPES = [(40, 1030), (1030, 40), (1, 1), (63, 65), (64, 64), (65, 63), (33, 31)]


@pytest.mark.parametrize("R_,C", TSHAPES)
def test_transpose_pack_bf16_and_transpose_f32(R_, C):
    """dst bf16 [C_pad][R_pad] = src^T bit for bit, exact +0.0 in every pad row and column, for C_pad = C and C + 3; NaN after
    src (a tile that reads past the last row shows as a NaN in a pad that must be zero), sentinel around dst.  rg_transpose_f32:
    bit-equal."""
    env = _Env()
    src64 = R.gauss((R_, C), 60 + R_)
    src64.view(-1)[0] = -0.0
    src = Guarded(src64.float(), NAN, after=64 * max(C, 64))
    want = src64.float().t().contiguous()
    Rp = ceil64(R_)
    for Cp in (C, C + 3):
        dst = Guarded(torch.full((Cp, Rp), SENTINEL, dtype=torch.float32).to(torch.bfloat16), SENTINEL)
        pattern16 = dst.flat[:1].view(torch.int16).item()
        env.ok(env.lib.rg_transpose_pack_bf16(_ptr(src.t), _ptr(dst.t), R_, C, Rp, Cp, env.stream), "rg_transpose_pack_bf16")
        d = dst.t.cpu()
        assert torch.equal(d[:C, :R_].contiguous().view(torch.int16), want.to(torch.bfloat16).contiguous().view(torch.int16))
        assert bool((d[:C, R_:].contiguous().view(torch.int16) == 0).all()), "pad columns (rows of src past R) are not +0.0"
        assert bool((d[C:, :].contiguous().view(torch.int16) == 0).all()), "pad rows (columns of src past C) are not +0.0"
        head, tail = dst.flat[:dst.before], dst.flat[dst.before + dst.n:]
        assert bool((head.view(torch.int16) == pattern16).all()) and bool((tail.view(torch.int16) == pattern16).all())
    out = _out((C, R_))
    env.ok(env.lib.rg_transpose_f32(_ptr(src.t), _ptr(out.t), R_, C, env.stream), "rg_transpose_f32")
    assert torch.equal(bits(out.t).cpu(), bits(want))
    assert out.surroundings_keep(SBITS)


# ================================================================== element-wise VAE kernels
@pytest.mark.parametrize("N,F,ld", [(3, 50, 64), (2, 64, 64), (12, 1030, 1088)])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_vae_dropout(N, F, ld, masked):
    """y = mask ? x * 2 : 0 bit for bit (a power-of-two scale is exact), +0.0 in the pad columns F..ld-1; NaN after x and after
    the mask's last byte is irrelevant (uint8), sentinel around y."""
    env = _Env()
    x64 = R.gauss((N, F), 70 + N)
    x = Guarded(x64.float(), NAN)
    gen = torch.Generator().manual_seed(71)
    mask = (torch.rand((N, F), generator=gen) < 0.5).to(torch.uint8)
    mg = Guarded(mask, 1)
    y = _out((N, ld))
    env.ok(env.lib.rg_vae_dropout(_ptr(x.t), _ptr(mg.t) if masked else 0, _ptr(y.t), N, F, ld, 2.0, env.stream), "rg_vae_dropout")
    want = x64.float() * 2.0
    if masked:
        want = torch.where(mask.bool(), want, torch.zeros_like(want))
    got = y.t.cpu()
    assert torch.isfinite(got).all()
    keep = mask.bool() if masked else torch.ones_like(mask).bool()
    assert torch.equal(bits(got[:, :F][keep]), bits(want[keep]))          # kept elements bit for bit
    assert bool((got[:, :F][~keep] == 0).all())
    if ld > F:
        _assert_pos_zero(y.t[:, F:], "dropout pad columns")
    assert y.surroundings_keep(SBITS)


NS = [1, 255, 257, 16384 * 256 + 3]                                        # the last: one element-wise grid sweep (16384 x 256) + 3


@pytest.mark.parametrize("n", NS)
def test_vae_reparam_forward_and_backward(n):
    """z = mu + eps exp(lv / 2) and its backward against fp64, element-wise within 4 fp32 rounding units (2^-24) of the largest
    term of each sum.  Derivation: a rounding is at most one unit of its result and expf is documented at 1 ulp = 2 units; the
    kernels form the products and the sum in fp64 and round once, so the error is 2 units of the exp term + 1 unit of the
    result, which is at most twice the largest term: 4.  (With every product and the sum rounded to fp32 the worst case is 6
    units; that form measured 4.36 at n = 16384 * 256 + 3 in the backward and 3.77 in the forward.)  lv in [-6, 6]: exp neither
    overflows nor underflows.  gmu = gmu_loss + gz is one fp32 addition: bit-equal.  gmu_loss / glv_loss each NULL and
    non-NULL."""
    env = _Env()
    mu, eps, gz, gml, glvl = (R.gauss((n,), 80 + i).float() for i in range(5))
    lv = R.finite_lv((n,), 86)
    after = 1024
    g = {k: Guarded(v, NAN, after=after) for k, v in dict(mu=mu, eps=eps, gz=gz, gml=gml, glvl=glvl, lv=lv).items()}
    z = _out((n,))
    env.ok(env.lib.rg_vae_reparam(_ptr(g["mu"].t), _ptr(g["lv"].t), _ptr(g["eps"].t), _ptr(z.t), n, env.stream), "rg_vae_reparam")
    ref, big = R.reparam_ref(mu.double(), lv.double(), eps.double())
    got = z.t.cpu().double()
    assert torch.isfinite(got).all()
    r = float(((got - ref).abs() / (4 * U32 * big)).max())
    print("RATIO rg_vae_reparam n=%d %.4f" % (n, r))
    assert r <= 1.0
    assert z.surroundings_keep(SBITS)
    for use_mu, use_lv in ((True, True), (False, True), (True, False), (False, False)):
        gmu, glv = _out((n,)), _out((n,))
        env.ok(env.lib.rg_vae_reparam_bwd(_ptr(g["gz"].t), _ptr(g["lv"].t), _ptr(g["eps"].t), _ptr(g["gml"].t) if use_mu else 0,
                                          _ptr(g["glvl"].t) if use_lv else 0, _ptr(gmu.t), _ptr(glv.t), n, env.stream),
               "rg_vae_reparam_bwd")
        rmu, rlv, big = R.reparam_bwd_ref(gz.double(), lv.double(), eps.double(), gml.double() if use_mu else None,
                                          glvl.double() if use_lv else None)
        assert torch.equal(gmu.t.cpu(), (gml + gz) if use_mu else gz), "gmu: not the fp32 sum"
        got = glv.t.cpu().double()
        assert torch.isfinite(got).all()
        r = float(((got - rlv).abs() / (4 * U32 * big)).max())
        print("RATIO rg_vae_reparam_bwd n=%d/mu%d/lv%d %.4f" % (n, use_mu, use_lv, r))
        assert r <= 1.0
        assert gmu.surroundings_keep(SBITS) and glv.surroundings_keep(SBITS)


@pytest.mark.parametrize("n", NS)
def test_add_inplace_and_tanh_inplace(n):
    env = _Env()
    a, b = R.gauss((n,), 90).float(), R.gauss((n,), 91).float()
    y, x = Guarded(a, SENTINEL), Guarded(b, NAN)
    env.ok(env.lib.rg_add_inplace(_ptr(y.t), _ptr(x.t), n, env.stream), "rg_add_inplace")
    assert torch.equal(bits(y.t).cpu(), bits(a + b)), "rg_add_inplace: not the fp32 sum"
    assert y.surroundings_keep(SBITS)
    t = R.gauss((n,), 92, 3.0).float()
    t[::7] = 0.0                                                           # the pad columns of the decoder output rely on tanh(0) == 0
    t[0] = 0.0
    tg = Guarded(t, SENTINEL)
    env.ok(env.lib.rg_tanh_inplace(_ptr(tg.t), n, env.stream), "rg_tanh_inplace")
    got = tg.t.cpu()
    assert bool((bits(got[t == 0]) == 0).all()), "tanh(0) is not +0.0"
    ul = R.ulps32(got.numpy(), np.tanh(t.double().numpy()))
    print("RATIO rg_tanh_inplace n=%d %.4f" % (n, float(ul.max()) / 2))
    assert float(ul.max()) <= 2.0, "tanh: %g units in the last place of fp64 tanh rounded to fp32" % float(ul.max())
    assert tg.surroundings_keep(SBITS)


# ================================================================== rg_vae_loss
@pytest.mark.parametrize("N,F,ld,Z", [(3, 50, 64, 8), (12, 1030, 1088, 136), (40, 19198, 19264, 16)])
def test_vae_loss(N, F, ld, Z):
    """Reconstruction: xr - x in {0, +-0.5, +-1} with zero pad columns makes sum d^2 exact in fp32 (4 N ld < 2^24, asserted), so
    the loss carries the rounding of inv_nf = 1 / (N F) and of one product: 3 * 2^-24 relative; g_recons = fl(2 / (N F)) d bit for
    bit (a power of two times an exact quotient times d).  The divisor is N F: with ld > F and a non-zero loss N ld would miss.
    KL against fp64 within L 2^-24 sum (1 + |l| + m^2 + e^l) / (2 N), L the longest addition path of the two-stage reduction
    + 4 (vae_fid_refs.loss_kl_path, from the launch geometry; <= 64 asserted).  g_mean / g_logvar within 4 rounding units of the
    largest term: the kernel forms beta / N and the products in fp64 and rounds once, which leaves expf's 2 units of e^l and one
    unit of the result (3 of max(e^l, 1) beta / 2N; 1 for g_mean).  training = 0: total == recons, KL gradients +-0.
    The last shape needs more than one sweep of the 1024 x 256-thread grid (770 560 elements)."""
    env = _Env()
    x, xr, mu, lv = R.loss_inputs(N, F, ld, Z, 100 + N)
    R.loss_exact_condition(x, xr, N, F, ld)
    L = R.loss_kl_path(N, ld, Z)
    assert L <= 64
    if N == 40:
        assert N * ld > 1024 * 256
    beta = float(np.float32(0.75))
    gx, gxr, gm, gl = (Guarded(t, NAN, after=2048) for t in (x, xr, mu, lv))
    wsb = env.lib.rg_vae_loss_workspace_bytes()
    assert wsb >= 2 * 1024 * 4
    for training in (1, 0):
        losses, g_rec, g_mu, g_lv = _out((3,)), _out((N, ld)), _out((N, Z)), _out((N, Z))
        ws = Guarded(torch.full((wsb // 4,), SENTINEL, dtype=torch.float32), SENTINEL)
        env.ok(env.lib.rg_vae_loss(_ptr(gx.t), _ptr(gxr.t), N, F, ld, _ptr(gm.t), _ptr(gl.t), Z, beta, training, _ptr(losses.t),
                                   _ptr(g_rec.t), _ptr(g_mu.t), _ptr(g_lv.t), _ptr(ws.t), wsb, env.stream), "rg_vae_loss")
        r = R.loss_ref(x[:, :F].double(), xr[:, :F].double(), mu.double(), lv.double(), beta, bool(training))
        total, recons, kl = (float(v) for v in losses.t.cpu().double())
        what = "vae_loss[%d x %d (ld %d) x %d, training=%d]" % (N, F, ld, Z, training)
        rr = abs(recons - float(r["recons"])) / (3 * U32 * float(r["recons"]))
        print("RATIO rg_vae_loss recons/%dx%d/t%d %.4f" % (N, F, training, rr))
        assert float(r["recons"]) > 0 and rr <= 1.0, what + ": reconstruction loss (divisor N F?)"
        lvd, mud = lv.double(), mu.double()
        kb = L * U32 * float((1 + lvd.abs() + mud * mud + lvd.exp()).sum()) / (2 * N)
        rk = abs(kl - float(r["kl"])) / kb
        print("RATIO rg_vae_loss kl/%dx%d/t%d %.4f" % (N, Z, training, rk))
        assert rk <= 1.0, what + ": KL term"
        if training:
            want = np.float32(recons) + np.float32(beta) * np.float32(kl)
            assert np.float32(total) == np.float32(want), what + ": total is not recons + beta * kl formed in fp32"
        else:
            assert total == recons, what + ": total != recons in evaluation"
        inv_nf = np.float32(1.0) / (np.float32(N) * np.float32(F))
        d32 = (xr - x)                                                     # exact
        want_g = torch.from_numpy((np.float32(2.0) * inv_nf) * d32.numpy())
        assert torch.equal(g_rec.t.cpu(), want_g), what + ": g_recons is not fl(2 / (N F)) (xr - x)"
        gmu, glv = g_mu.t.cpu().double(), g_lv.t.cpu().double()
        if training:
            um = float(((gmu - r["g_mean"]).abs() / (4 * U32 * r["g_mean"].abs()).clamp_min(1e-300)).max())
            big = beta * 0.5 * torch.maximum(lvd.exp(), torch.ones_like(lvd)) / N
            ul = float(((glv - r["g_logvar"]).abs() / (4 * U32 * big)).max())
            print("RATIO rg_vae_loss g_mean/%dx%d %.4f" % (N, Z, um))
            print("RATIO rg_vae_loss g_logvar/%dx%d %.4f" % (N, Z, ul))
            assert um <= 1.0 and ul <= 1.0, what + ": KL gradients"
        else:
            assert bool((gmu == 0).all()) and bool((glv == 0).all()), what + ": KL gradients flow in evaluation"
        for o in (losses, g_rec, g_mu, g_lv, ws):
            assert o.surroundings_keep(SBITS), what + ": wrote outside an output / the workspace"


# ================================================================== Inception data movement
WINDOWS = [(3, 3, 2, 2, 0, 0), (3, 3, 1, 1, 1, 1), (5, 5, 1, 1, 2, 2), (1, 7, 1, 1, 0, 3), (7, 1, 1, 1, 3, 0),
           (1, 3, 1, 1, 0, 1), (3, 1, 1, 1, 1, 0)]
# (C, ldx): float4 path; float4 path inside a wider pitch; scalar path; C % 4 == 0 but the pitch is not (must go scalar); C = 3
IM2COL_LAYOUTS = [(8, 8), (8, 12), (6, 6), (4, 6), (3, 3)]


@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "k%dx%d_s%d%d_p%d%d" % w)
def test_im2col_nhwc(win):
    """cols bit-equal to the index-arithmetic reference (zeros outside the image) on N = 2, 9 x 7, every channel layout; x sits
    between NaN guards of one image each (a border tap that is READ instead of zero-filled shows; the pointer may be formed
    but not dereferenced) and the columns of a wider pitch that are not the operand are NaN too; sentinel after cols."""
    env = _Env()
    kh, kw, sh, sw, ph, pw = win
    N, H, W = 2, 9, 7
    for C, ldx in IM2COL_LAYOUTS:
        x64 = R.gauss((N, H, W, C), 110 + C + ldx)
        xbuf = torch.full((N, H, W, ldx), NAN, dtype=torch.float32)
        xbuf[..., :C] = x64.float()
        xg = Guarded(xbuf, NAN, before=N * H * W * 12 // 64 * 64 + 64, after=N * H * W * 12)
        want = torch.from_numpy(R.im2col_ref(x64.float().numpy(), kh, kw, sh, sw, ph, pw))
        cols = _out(tuple(want.shape))
        env.ok(env.lib.rg_im2col_nhwc(_ptr(xg.t), ldx, _ptr(cols.t), N, H, W, C, kh, kw, sh, sw, ph, pw, env.stream),
               "rg_im2col_nhwc")
        got = cols.t.cpu()
        what = "im2col_nhwc[C=%d, ldx=%d]" % (C, ldx)
        assert torch.isfinite(got).all(), what + ": a tap outside the image (or outside the channel slice) was read"
        assert torch.equal(bits(got), bits(want)), what
        assert cols.surroundings_keep(SBITS), what + ": wrote outside cols"


@pytest.mark.parametrize("H,W", [(9, 7), (8, 8)])
def test_pool2d_nhwc(H, W):
    """max 3 / 2 / 0 (on 8 x 8 the last window does not reach the edge) bit-equal, all-negative inputs included; avg 3 / 1 / 1 with
    divisor 9 at corners and edges.  The average's inputs are multiples of 2^-8 up to 4, so its sum is exact in fp32 and the one
    rounding is the division: gated at 2 rounding units (2 * 2^-24 relative) of the fp64 reference.  C = 5, read from a slice
    of a wider NaN-filled row (ldx = 8, offset 2) and written into a slice of a sentinel row (ldy = 11, offset 3)."""
    env = _Env()
    N, C, ldx, c0, ldy, d0 = 2, 5, 8, 2, 11, 3
    for mode, k, s, p, x64 in ((0, 3, 2, 0, R.gauss((N, H, W, C), 120)), (0, 3, 2, 0, -R.gauss((N, H, W, C), 121).abs() - 1.0),
                               (1, 3, 1, 1, R.dyadic((N, H, W, C), 122))):
        x64 = x64.float().double()
        xbuf = torch.full((N, H, W, ldx), NAN, dtype=torch.float32)
        xbuf[..., c0:c0 + C] = x64.float()
        xg = Guarded(xbuf, NAN, before=N * H * W * ldx // 64 * 64 + 64, after=N * H * W * ldx)
        ref = torch.from_numpy(R.pool_ref(x64.numpy(), k, s, p, mode))
        Ho, Wo = ref.shape[1], ref.shape[2]
        y = _out((N, Ho, Wo, ldy))
        env.ok(env.lib.rg_pool2d_nhwc(xg.t.data_ptr() + 4 * c0, ldx, y.t.data_ptr() + 4 * d0, ldy, N, H, W, C, k, s, p, mode,
                                      env.stream), "rg_pool2d_nhwc")
        got = y.t[..., d0:d0 + C].cpu()
        what = "pool2d_nhwc[mode %d, %d x %d]" % (mode, H, W)
        assert torch.isfinite(got).all(), what + ": read outside the image or the channel slice"
        if mode == 0:
            assert torch.equal(bits(got), bits(ref.float())), what
        else:
            err = (got.double() - ref).abs()
            assert bool((err <= 2 * U32 * ref.abs()).all()), what + ": worst %g units" % float((err / (U32 * ref.abs()).clamp_min(1e-300)).max())
            print("RATIO rg_pool2d_nhwc avg%dx%d %.4f" % (H, W, float((err / (2 * U32 * ref.abs()).clamp_min(1e-300)).max())))
        _assert_sentinel(y.t[..., :d0], what + " channels below the slice")
        _assert_sentinel(y.t[..., d0 + C:], what + " channels above the slice")
        assert y.surroundings_keep(SBITS), what + ": wrote outside y"


def test_nchw_to_nhwc_affine():
    """y[n][p][c] = x[n][c][p] scale[c] + shift[c] as ONE fused multiply-add: one rounding, so at most one unit 2^-24 of the
    result.  (A separately rounded product is a second unit, of |x s|: that form measured 1.20 units of |x s| + |shift|.)"""
    env = _Env()
    N, C, H, W = 2, 3, 5, 4
    x64, sc64, sh64 = R.gauss((N, C, H, W), 130).float().double(), R.gauss((C,), 131).float().double(), R.gauss((C,), 132).float().double()
    x, sc, sh = Guarded(x64.float(), NAN), Guarded(sc64.float(), NAN), Guarded(sh64.float(), NAN)
    y = _out((N, H, W, C))
    env.ok(env.lib.rg_nchw_to_nhwc_affine(_ptr(x.t), _ptr(y.t), N, C, H, W, _ptr(sc.t), _ptr(sh.t), env.stream),
           "rg_nchw_to_nhwc_affine")
    xs = x64.permute(0, 2, 3, 1) * sc64
    ref, unit = xs + sh64, (U32 * (xs + sh64).abs()).clamp_min(2.0 ** -149)
    got = y.t.cpu().double()
    assert torch.isfinite(got).all()
    r = float(((got - ref).abs() / unit).max())
    print("RATIO rg_nchw_to_nhwc_affine 2x3x5x4 %.4f" % r)
    assert r <= 1.0
    assert y.surroundings_keep(SBITS)


@pytest.mark.parametrize("N,HW,C", [(3, 64, 10), (3, 1, 10), (1, 64, 257)])
def test_spatial_mean_nhwc(N, HW, C):
    """mean over HW in order: HW - 1 additions and a division, each at most a unit of sum |x|, so |err| <= HW 2^-24 mean |x|.
    N C = 257: the second block of 256 threads is ragged.  HW = 1: the value itself."""
    env = _Env()
    x64 = R.gauss((N, HW, C), 140 + C).float().double()
    x = Guarded(x64.float(), NAN, after=HW * C + 256)
    y = _out((N, C))
    env.ok(env.lib.rg_spatial_mean_nhwc(_ptr(x.t), _ptr(y.t), N, HW, C, env.stream), "rg_spatial_mean_nhwc")
    got = y.t.cpu().double()
    assert torch.isfinite(got).all()
    ref, bnd = x64.mean(1), HW * U32 * x64.abs().mean(1)
    r = float(((got - ref).abs() / bnd).max())
    print("RATIO rg_spatial_mean_nhwc %dx%dx%d %.4f" % (N, HW, C, r))
    assert r <= 1.0
    if HW == 1:
        assert torch.equal(y.t.cpu(), x64[:, 0].float())
    assert y.surroundings_keep(SBITS)
