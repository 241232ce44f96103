"""The fp32 mode's plane kernels op by op, through the C ABI of the bf16 build (rg_split_planes, rg_f32p_conv with
rg_mfma_conv_up_planes64 behind it, rg_f32p_wgrad): the kernels are handed planes the test built itself, so exact arithmetic sees
what Gaussian operands under max|err| <= tol max|ref| (tests/test_f32_planes_gpu.py) cannot.  References, operand builders and
case tables are in tests/f32_planes_refs.py; tests/test_f32_planes_refs_cpu.py checks every condition on the same operands.

(a) PAIR TABLE   one-hot planes, all nine placements, both tiers: ref(X, W) for a pair of the tier, exactly zero otherwise.
(b) SWEEP        all-live planes with nine distinct power-of-two pair weights, torch.equal: row tails, rectangular planes, two
                 channel blocks per tap, several column tiles, split and unsplit (read from the planner's queries), k order and
                 XCD order; the 64-column transposed conv also with its fused mask.
(c) STATISTICS   unit-weight planes: the BatchNorm column sums of the unsplit fp32 epilogue, exact, rows of a tail tile included.
(d) WGRAD        all-live planes: wgrad8_blocks in {1, 8, 256}, one and two segments, accumulate on and off, an odd count of
                 pixel tiles, the narrowest channel counts.
(e) SPLIT        rg_split_planes bit for bit against its definition, through the grid-stride wrap.
(f) CONTRACTS    *_supported at the edges of the rule, RG_EWORKSPACE, RG_EINVAL, RG_EUNSUPPORTED: host side only.
(g) HIPOPS       Gaussian operands through HipOps at the tail shapes and one unsplit shape, against fp64 (the tolerances of
                 tests/test_f32_planes_gpu.py); the measured maxima are printed as "ERR <op> <case> <products> <value>"
                 (profiles/f32_planes_op_errors.txt records them).
Every output, workspace and statistics buffer is exactly as large as its query says, inside a pattern-filled allocation whose
surroundings must keep the pattern; operands sit inside NaN.
"""
import math

import pytest
import torch

import f32_planes_refs as R
from guarded import DEV, SBITS, Guarded
from test_ops_exact_gpu import _Options, ref_down, ref_up, ref_wgrad
from vae_fid_refs import SENTINEL, bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENT16 = -24704.0                                   # 0xc6c1 as bf16
RG_EINVAL, RG_EUNSUPPORTED, RG_EWORKSPACE = -1, -2, -3
_ENV = []


class _Env:
    def __init__(self):
        from rna_gan_amd import _abi
        from rna_gan_amd.ops_hip import HipOps
        self.abi = _abi
        self.ops = HipOps(torch.float32, DEV)        # fp32 storage runs on the bf16 build of the library
        self.lib = self.ops.lib
        assert self.ops.H16 == _abi.RG_BF16

    @property
    def stream(self):
        return self.ops.stream


def _env():
    if not _ENV:
        _ENV.append(_Env())
    return _ENV[0]


def _guard(shape, dtype, fill, after=4096):
    """a guarded.Guarded built on the device (no host image of a large buffer)"""
    g = Guarded.__new__(Guarded)
    n = int(math.prod(shape))
    g.before, g.n = 128, n
    g.flat = torch.full((g.before + n + after,), fill, dtype=dtype, device=DEV)
    g.t = g.flat[g.before:g.before + n].view(shape)
    return g


def _operand(planes):
    """[3, ...] planes as bf16 inside NaN (the kernels' buffer descriptors end at 3 planes: nothing beyond may be read)"""
    g = _guard(tuple(planes.shape), torch.bfloat16, NAN)
    g.t.copy_(planes.to(DEV))
    assert torch.equal(g.t.float().cpu(), planes.float().cpu()), "the planes are bf16 numbers"
    return g


def _out(shape, init=None):
    g = _guard(tuple(shape), torch.float32, SENTINEL)
    if init is not None:
        g.t.copy_(init.to(DEV))
    return g


def _wup(E, wdn):
    """the transposed conv's operand image wup[3][16][I][O] of wdn planes [3][O][16][I], plane by plane (HipOps._plane_packs)"""
    _, O, _, _, I = wdn.t.shape
    g = _guard((3, 16, I, O), torch.bfloat16, NAN)
    for p in range(3):
        E.abi.check(E.lib.rg_pack_conv_wup_from_bf16(wdn.t[p].data_ptr(), g.t[p].data_ptr(), O, I, E.stream), "rg_pack_conv_wup_from_bf16")
    return g


def _state(E, up, dims, products):
    """what the planner gives this launch: 'split', 'unsplit' (a tiled kernel writing statistics rows) or 'up64'"""
    wsb = int(E.lib.rg_f32p_conv_workspace_bytes(up, *dims, products))
    rows = int(E.lib.rg_f32p_conv_stats_rows(up, *dims, products))
    if wsb:
        assert rows == 0
        return "split"
    if rows:
        return "unsplit"
    assert up and E.lib.rg_f32p_conv_mask_supported(up, *dims, products) == 1
    return "up64"


class _Conv:
    """one conv case on the device: operands once, then launches with every buffer at its queried size"""

    def __init__(self, E, kernel, dims, A, B):
        self.E, self.kernel, self.dims = E, kernel, dims
        self.up = 1 if R.KERNELS[kernel][0] == "up" else 0
        N, Hl, Wl, O, I = dims
        self.x = _operand(A)
        self.wdn = _operand(B)
        self.w = _wup(E, self.wdn) if self.up else self.wdn
        self.yshape = (N, 2 * Hl, 2 * Wl, I) if self.up else (N, Hl, Wl, O)
        self.y = _out(self.yshape)

    def run(self, products, stats=False, mask=None, slope=1.0, expect=0):
        E, lib, dims = self.E, self.E.lib, self.dims
        assert lib.rg_f32p_conv_supported(self.up, *dims, products) == 1, "%s %s: not supported" % (self.kernel, dims)
        wsb = int(lib.rg_f32p_conv_workspace_bytes(self.up, *dims, products))
        rows = int(lib.rg_f32p_conv_stats_rows(self.up, *dims, products))
        ws = _guard((wsb // 4,), torch.float32, SENTINEL, after=8192) if wsb else None
        st = _out((rows if rows else 4, 2, self.yshape[-1])) if stats else None
        self.y.t.fill_(SENTINEL)
        rc = lib.rg_f32p_conv(self.up, self.x.t.data_ptr(), self.w.t.data_ptr(), self.y.t.data_ptr(), *dims, products,
                              st.t.data_ptr() if st else None, mask.data_ptr() if mask is not None else None, float(slope),
                              ws.t.data_ptr() if ws else None, wsb, E.stream)
        torch.cuda.synchronize()
        assert rc == expect, "rg_f32p_conv returned %d" % rc
        what = "%s %s, %d products" % (self.kernel, dims, products)
        assert self.y.surroundings_keep(SBITS), what + ": wrote outside y"
        assert ws is None or ws.surroundings_keep(SBITS), what + ": wrote outside the workspace"
        assert st is None or st.surroundings_keep(SBITS), what + ": wrote outside the statistics rows"
        return self.y.t, (st.t if st else None), rows


def _exact(got, ref, what):
    ref = ref.to(got.device).float()
    assert torch.equal(got, ref), "%s: %d of %d outputs differ, first at %s" % (
        what, int((got != ref).sum()), ref.numel(), (got != ref).nonzero()[:4].tolist())


# ------------------------------------------------------------------ (a) pair table
@pytest.mark.parametrize("kernel", [k for k in R.PAIR_TABLE if not k.startswith("wgrad")])
def test_conv_pair_table(kernel):
    E, dims = _env(), R.PAIR_TABLE[kernel]
    op = R.KERNELS[kernel][0]
    for p in range(3):
        for q in range(3):
            A, B, ref = R.one_hot(op, dims, p, q)
            c = _Conv(E, kernel, dims, A, B)
            for products in (6, 3):
                y, _, _ = c.run(products)
                want = ref if (p, q) in R.PAIRS[products] else torch.zeros_like(ref)
                _exact(y, want, "%s: X in plane %d, W in plane %d, %d products" % (kernel, p, q, products))


@pytest.mark.parametrize("kernel", ["wgrad_wide", "wgrad_narrow"])
def test_wgrad_pair_table(kernel):
    E, dims = _env(), R.PAIR_TABLE[kernel]
    for p in range(3):
        for q in range(3):
            A, B, ref = R.one_hot("wgrad", dims, p, q)
            lo, hi = _operand(A), _operand(B)
            for products in (6, 3):
                want = ref if (p, q) in R.PAIRS[products] else torch.zeros_like(ref)
                dw = _wgrad(E, dims, products, [lo], [hi], None, 0)
                _exact(dw, want, "%s: low in plane %d, high in plane %d, %d products" % (kernel, p, q, products))


# ------------------------------------------------------------------ (b) exact sweep
def test_sweep_covers_every_kernel_split_and_unsplit_with_a_row_tail():
    """read from the planner's own queries (no launch): each tiled kernel is swept split and unsplit, and both with a partial row
    tile; the 64-column kernel is never split"""
    E = _env()
    seen = {}
    for kernel, dims in R.SWEEP_CASES:
        up, bm = (1 if R.KERNELS[kernel][0] == "up" else 0), R.KERNELS[kernel][1]
        tail = (dims[0] * dims[1] * dims[2]) % bm != 0
        for products in (6, 3):
            seen.setdefault(kernel, set()).add((_state(E, up, dims, products), tail, products))
    for kernel in ("down256", "down512", "up256", "up512"):
        for products in (6, 3):
            for state in ("split", "unsplit"):
                for tail in (True, False) if state == "split" else (True,):
                    assert (state, tail, products) in seen[kernel], "%s is not swept %s, tail %s, %d products" % (kernel, state, tail, products)
    assert {s for s, _, _ in seen["up64"]} == {"up64"} and {t for _, t, _ in seen["up64"]} == {True, False}
    for kernel, dims in R.UNSPLIT.items():
        for products in (6, 3):
            assert _state(E, 1 if R.KERNELS[kernel][0] == "up" else 0, dims, products) == "unsplit"


@pytest.mark.parametrize("kernel,dims", R.SWEEP_CASES, ids=R.case_id)
def test_conv_exact_sweep(kernel, dims):
    E = _env()
    op = R.KERNELS[kernel][0]
    A, B = R.sweep_operands(kernel, dims)
    c = _Conv(E, kernel, dims, A, B)
    Ad, Bd = A.to(DEV), B.to(DEV)
    for products in (6, 3):
        ref = R.live_reference(op, Ad, Bd, products, what=str(dims))          # (conditions asserted again, on the device)
        state = _state(E, c.up, dims, products)
        if dims == R.UNSPLIT.get(kernel):
            assert state == "unsplit" and int(E.lib.rg_f32p_conv_stats_rows(c.up, *dims, products)) > 0
        for korder in (0, 1):
            for xcd in (0, 1):
                with _Options(E.lib, korder=korder, xcd=xcd):
                    y, _, _ = c.run(products)
                    _exact(y, ref, "%s %s (%s), %d products, korder %d, xcd %d" % (kernel, dims, state, products, korder, xcd))


@pytest.mark.parametrize("dims", R.MASK_CASES, ids=R.case_id)
def test_conv_up64_fused_mask(dims):
    E = _env()
    A, B, m, f = R.mask_operands(dims)
    c = _Conv(E, "up64", dims, A, B)
    mg = _guard(tuple(m.shape), torch.float32, NAN)
    mg.t.copy_(m.to(DEV))
    assert torch.equal(bits(mg.t).cpu(), bits(m)), "the mask keeps its signed zeros"
    for products in (6, 3):
        assert E.lib.rg_f32p_conv_mask_supported(1, *dims, products) == 1
        ref = R.live_reference("up", A.to(DEV), B.to(DEV), products, L=R.L_MASK, factor=f.to(DEV), what="masked " + str(dims))
        for korder in (0, 1):
            with _Options(E.lib, korder=korder):
                y, _, _ = c.run(products, mask=mg.t, slope=R.SLOPE)
                _exact(y, ref, "up64 %s masked, %d products, korder %d" % (dims, products, korder))


def test_conv_refuses_a_mask_where_it_is_not_fused():
    """a shape fplan takes (a tiled kernel): RG_EUNSUPPORTED, nothing written"""
    E, dims = _env(), R.PAIR_TABLE["up256"]
    A, B, _ = R.one_hot("up", dims, 0, 0)
    c = _Conv(E, "up256", dims, A, B)
    m = torch.ones(c.yshape, device=DEV)
    for products in (6, 3):
        assert E.lib.rg_f32p_conv_mask_supported(1, *dims, products) == 0
        y, _, _ = c.run(products, mask=m, slope=R.SLOPE, expect=RG_EUNSUPPORTED)
        assert bool((bits(y) == SBITS).all())


# ------------------------------------------------------------------ (c) statistics epilogue
@pytest.mark.parametrize("kernel,dims,products", R.STATS_CASES, ids=R.case_id)
def test_conv_statistics_epilogue(kernel, dims, products):
    E = _env()
    op = R.KERNELS[kernel][0]
    A, B = R.stats_operands(kernel, dims, products)
    c = _Conv(E, kernel, dims, A, B)
    y_ref, sums = R.unit_reference(op, A.to(DEV), B.to(DEV), products, what=kernel + str(dims))
    y, st, rows = c.run(products, stats=True)
    assert rows > 0 and st.shape == (rows, 2, y_ref.shape[-1]), "an unsplit launch of a tiled kernel"
    _exact(y, y_ref, "%s %s" % (kernel, dims))
    assert not bool((bits(st) == SBITS).any()), "every statistics row is written"
    got = st.double().sum(0)
    assert torch.equal(got[0], sums[0]), "column sums of y: %d columns differ" % int((got[0] != sums[0]).sum())
    assert torch.equal(got[1], sums[1]), "column sums of y^2: %d columns differ" % int((got[1] != sums[1]).sum())
    _exact(c.run(products)[0], y_ref, "%s %s without statistics" % (kernel, dims))


def test_split_conv_leaves_the_statistics_pointer_alone():
    E = _env()
    for kernel, dims in (("down256", (5, 8, 8, 256, 64)), ("up512", (2, 16, 16, 128, 128))):
        A, B = R.sweep_operands(kernel, dims)
        c = _Conv(E, kernel, dims, A, B)
        for products in (6, 3):
            assert _state(E, c.up, dims, products) == "split"
            y, st, rows = c.run(products, stats=True)
            assert rows == 0 and bool((bits(st) == SBITS).all()), "a split launch wrote statistics"
            _exact(y, R.planes_expected(R.KERNELS[kernel][0], A, B, products), "%s %s" % (kernel, dims))


# ------------------------------------------------------------------ (d) weight gradient
def _wgrad(E, dims, products, lows, highs, dw_init, accumulate, expect=0, short=0):
    """one rg_f32p_wgrad launch: dw preset to dw_init (overwritten or added to), the workspace exactly what the query says"""
    lib = E.lib
    N, Hl, Wl, O, I = dims
    two = len(lows) == 2
    assert lib.rg_f32p_wgrad_supported(*dims, products) == 1
    wsb = int(lib.rg_f32p_wgrad_workspace_bytes(*dims, products, int(two)))
    ws = _guard((wsb // 4,), torch.float32, SENTINEL, after=8192) if wsb else None
    dw = _out((O, 4, 4, I), init=dw_init.float() if dw_init is not None else None)
    rc = lib.rg_f32p_wgrad(lows[0].t.data_ptr(), highs[0].t.data_ptr(), lows[1].t.data_ptr() if two else None,
                           highs[1].t.data_ptr() if two else None, dw.t.data_ptr(), *dims, products, int(accumulate),
                           ws.t.data_ptr() if ws else None, wsb - short, E.stream)
    torch.cuda.synchronize()
    assert rc == expect, "rg_f32p_wgrad returned %d" % rc
    assert dw.surroundings_keep(SBITS), "wrote outside dw"
    assert ws is None or ws.surroundings_keep(SBITS), "wrote outside the workspace"
    dw.split = wsb > 0
    return dw.t


@pytest.mark.parametrize("kernel,dims", R.WGRAD_CASES, ids=R.case_id)
def test_wgrad_exact(kernel, dims):
    E = _env()
    splits = set()
    for two in (False, True):
        A, B, dw0 = R.wgrad_operands(dims, two)
        lows, highs = [_operand(a) for a in A], [_operand(b) for b in B]
        Ad, Bd = [a.to(DEV) for a in A], [b.to(DEV) for b in B]
        for products in (6, 3):
            ref = R.live_reference("wgrad", Ad, Bd, products, L=R.L_WGRAD, what="%s, %d segments" % (dims, len(A)))
            for blocks in (1, 8, 256):
                with _Options(E.lib, wgrad8_blocks=blocks):
                    splits.add(int(E.lib.rg_f32p_wgrad_workspace_bytes(*dims, products, int(two))) > 0)
                    for acc in (0, 1):
                        dw = _wgrad(E, dims, products, lows, highs, dw0, acc)
                        _exact(dw, ref + dw0.to(DEV) if acc else ref, "%s %s: %d segments, %d products, wgrad8_blocks %d, accumulate %d" % (
                            kernel, dims, len(A), products, blocks, acc))
    assert splits == {False, True}, "the case runs the direct write (in-kernel accumulate) and the split-K slabs"


# ------------------------------------------------------------------ (e) rg_split_planes
def _split(E, v, expect=0, src_off=0, dst_off=0, n=None):
    """v (CPU fp32) -> ([3][n] bf16 bit patterns from the device, the guarded destination)"""
    n = v.numel() if n is None else n
    src = _guard((v.numel() + 8,), torch.float32, NAN)
    src.t[src_off:src_off + v.numel()].copy_(v.to(DEV))
    dst = _guard((3 * v.numel() + 16,), torch.bfloat16, SENT16)
    rc = E.lib.rg_split_planes(src.t.data_ptr() + 4 * src_off, dst.t.data_ptr() + 2 * dst_off, n, E.stream)
    torch.cuda.synchronize()
    assert rc == expect, "rg_split_planes returned %d" % rc
    return dst


def _sent16(t):
    return t.view(torch.int16) == torch.tensor(SENT16, dtype=torch.bfloat16).view(torch.int16).item()


def _planes_of(dst, n):
    assert bool(_sent16(dst.flat[:dst.before]).all()) and bool(_sent16(dst.flat[dst.before + 3 * n:]).all()), "wrote outside the planes"
    return dst.t[:3 * n].view(3, n).view(torch.int16)


@pytest.mark.parametrize("n", [8, 2 ** 24 + 2056], ids=["n8", "grid_stride_wrap"])
def test_split_planes_bit_for_bit(n):
    """every plane against split_ref on the structured set (every exponent 2^-100 .. 2^127 x the low-mantissa patterns with
    both round-to-even ties x both signs, +-0, +-inf, NaN by class, +-3.4e38); n = 2^24 + 2056 is past one sweep of the
    8192-block grid"""
    E = _env()
    vals = R.structured_values()
    v = R.tiled(vals, n)
    if n == 8:
        v[7] = vals[7 + 2 * (100 * 7 + 3)]                   # 1.0 + 2^-8: a tie
    want = R.split_ref(v).view(torch.int16)
    got = _planes_of(_split(E, v), n).cpu()
    # a NaN has no rounding: its h must be a NaN (of the same sign) with zero residual planes -- which payload the conversion
    # gives it is printed, not compared (the device gives 0x7fc0; torch's CPU cast, the reference, not the same on every host);
    # everything else is compared bit for bit
    nan = torch.isnan(v)
    assert bool(nan.any()) and bool(torch.isnan(got[0].view(torch.bfloat16).float()[nan]).all()), "h of a NaN is not a NaN"
    assert bool(((got[0][nan] < 0) == (v[nan].view(torch.int32) < 0)).all())
    print("NAN rg_split_planes: h of 0x%08x is %s" % (int(v[nan][0].view(torch.int32)) & 0xffffffff,
                                                      sorted({"0x%04x" % (int(b) & 0xffff) for b in got[0][nan].unique()})))
    got[0][nan] = want[0][nan]
    for k, name in enumerate("hml"):
        bad = got[k] != want[k]
        assert not bool(bad.any()), "plane %s: %d of %d differ, first at %s (v = %s)" % (
            name, int(bad.sum()), n, bad.nonzero()[:4].flatten().tolist(), v[bad][:4].tolist())


def test_split_planes_tiny_values_are_reported():
    """|v| < 2^-100: the residual planes can be bf16 subnormals.  What the conversion does there is printed (and recorded in
    profiles/f32_planes_op_errors.txt), not asserted: HipOps' claim v = h + m + l starts at 1e-30."""
    E = _env()
    v = R.tiny_values()
    v = R.tiled(v, (v.numel() + 7) // 8 * 8)
    want = R.split_ref(v)
    got = _planes_of(_split(E, v), v.numel()).cpu()
    sub = (want.float().abs() < 2.0 ** -126) & (want.float() != 0)
    diff = got != want.view(torch.int16)
    flushed = diff & (got.view(torch.bfloat16).float() == 0)
    s = got.view(torch.bfloat16).double().sum(0)
    print("TINY rg_split_planes: %d values, %d plane entries subnormal in the reference; planes differing h/m/l = %s, of which stored "
          "as zero = %s; h + m + l == v for %d of %d" % (v.numel(), int(sub.sum()), diff.sum(1).tolist(), flushed.sum(1).tolist(),
                                                         int((s == v.double()).sum()), v.numel()))
    assert bool(torch.isfinite(got.view(torch.bfloat16).float()).all())


def test_split_planes_refuses_bad_arguments_without_a_launch():
    E = _env()
    v = R.tiled(R.structured_values(), 64)
    for kw in ({"n": 12}, {"n": 0}, {"src_off": 1}, {"dst_off": 4}):        # n % 8, n = 0, src / dst not 16-byte aligned
        dst = _split(E, v[:32] if "src_off" in kw else v, expect=RG_EINVAL, **kw)
        assert bool(_sent16(dst.flat).all()), "rg_split_planes(%s) launched" % kw
    assert E.lib.rg_split_planes(None, 0, 8, E.stream) == RG_EINVAL


# ------------------------------------------------------------------ (f) host-side contracts (no launch, no large allocation)
G = 0x7fffff00


def test_conv_supported_rule():
    lib = _env().lib
    for products in (6, 3):
        for up in (0, 1):
            O, I = (64, 256) if up else (256, 64)
            ok = lambda N, Hl, Wl, O=O, I=I, pr=products: lib.rg_f32p_conv_supported(up, N, Hl, Wl, O, I, pr)
            assert ok(1, 16, 16) == 1 and ok(1, 8, 16) == 0                   # M >= 256
            narrow = {"O": 64, "I": 128} if up else {"O": 128, "I": 64}
            assert ok(2, 16, 16, **narrow) == 1 and ok(1, 16, 16, **narrow) == 0                  # the 512 x 128 tile: M >= 512
            assert ok(4, 12, 16) == 0 and ok(4, 16, 12) == 0 and ok(3, 16, 16) == 1               # plane sides are powers of two, N is free
            assert ok(1, 16, 16, **({"O": 192} if up else {"I": 192})) == 0                       # Cin / 64 a power of two
            assert ok(1, 16, 16, **({"O": 128} if up else {"I": 128})) == 1
            assert ok(0, 16, 16) == 0
            for bad in (0, 1, 2, 4, 5, 9, -3):
                assert lib.rg_f32p_conv_supported(up, 1, 16, 16, O, I, bad) == 0
        assert lib.rg_f32p_conv_supported(1, 1, 16, 16, 64, 64, products) == 1 and lib.rg_f32p_conv_supported(0, 1, 16, 16, 64, 64, products) == 0
        assert lib.rg_f32p_conv_supported(1, 1, 8, 16, 64, 64, products) == 0 and lib.rg_f32p_conv_supported(1, 1, 16, 16, 96, 64, products) == 0
        # the 2 GB guards: 3 planes of an operand stay below 0x7fffff00 bytes (arithmetic only)
        a = lambda N: 3 * N * 64 * 64 * 4 * 64 * 2                           # conv, I = 64 at 64 x 64
        assert a(341) < G <= a(342)
        assert lib.rg_f32p_conv_supported(0, 341, 64, 64, 256, 64, products) == 1 and lib.rg_f32p_conv_supported(0, 342, 64, 64, 256, 64, products) == 0
        a = lambda N: 3 * N * 64 * 64 * 256 * 2                              # transposed conv, O = 256
        assert a(341) < G <= a(342)
        assert lib.rg_f32p_conv_supported(1, 341, 64, 64, 256, 256, products) == 1 and lib.rg_f32p_conv_supported(1, 342, 64, 64, 256, 256, products) == 0
        b = lambda O: 3 * O * 16 * 4096 * 2                                  # the weights, I = 4096
        assert b(5376) < G <= b(5504)
        for up in (0, 1):
            O, I = (4096, 5376) if up else (5376, 4096)
            assert lib.rg_f32p_conv_supported(up, 2, 16, 16, O, I, products) == 1
            O, I = (4096, 5504) if up else (5504, 4096)
            assert lib.rg_f32p_conv_supported(up, 2, 16, 16, O, I, products) == 0
        a = lambda N: 3 * N * 64 * 64 * 64 * 2                               # the 64-column transposed conv, O = 64
        assert a(1365) < G <= a(1366)
        assert lib.rg_f32p_conv_supported(1, 1365, 64, 64, 64, 64, products) == 1 and lib.rg_f32p_conv_supported(1, 1366, 64, 64, 64, 64, products) == 0
        assert lib.rg_f32p_conv_mask_supported(1, 1365, 64, 64, 64, 64, products) == 1 and lib.rg_f32p_conv_mask_supported(1, 1366, 64, 64, 64, 64, products) == 0


def test_wgrad_supported_rule():
    lib = _env().lib
    for products in (6, 3):
        ok = lambda N, Hl, Wl, O=256, I=16, pr=products: lib.rg_f32p_wgrad_supported(N, Hl, Wl, O, I, pr)
        assert ok(1, 16, 16) == 1 and ok(1, 8, 16) == 0 and ok(5, 8, 8) == 1 and ok(0, 16, 16) == 0     # K >= 256, K % 64 == 0
        assert ok(4, 12, 16) == 0 and ok(4, 16, 12) == 0
        assert ok(1, 16, 16, I=8) == 0 and ok(1, 16, 16, I=24) == 0 and ok(1, 16, 16, I=48) == 1          # wide: 16 I % 256 == 0
        assert ok(1, 16, 16, O=128, I=16) == 0 and ok(1, 16, 16, O=128, I=32) == 1 and ok(1, 16, 16, O=384, I=48) == 0   # narrow: 16 I % 512
        assert ok(1, 16, 16, O=192, I=32) == 0
        for bad in (0, 1, 2, 4, 5, 9, -3):
            assert ok(1, 16, 16, pr=bad) == 0
        lo = lambda N, O: 3 * N * 64 * 64 * O * 2
        hi = lambda N, I: 3 * N * 64 * 64 * 4 * I * 2
        assert lo(170, 512) < G <= lo(171, 512) and hi(171, 16) < G                                      # the `low` guard alone
        assert ok(170, 64, 64, O=512, I=16) == 1 and ok(171, 64, 64, O=512, I=16) == 0
        assert hi(170, 128) < G <= hi(171, 128) and lo(171, 128) < G                                     # the `high` guard alone
        assert ok(170, 64, 64, O=128, I=128) == 1 and ok(171, 64, 64, O=128, I=128) == 0


def test_workspace_one_byte_short_and_half_a_second_segment_are_refused():
    E = _env()
    lib = E.lib
    dims = (5, 8, 8, 256, 64)
    A, B = R.sweep_operands("down256", dims)
    c = _Conv(E, "down256", dims, A, B)
    for products in (6, 3):
        wsb = int(lib.rg_f32p_conv_workspace_bytes(0, *dims, products))
        assert wsb == 4 * 320 * 256 * (wsb // (4 * 320 * 256)) and wsb > 0
        ws = _out((wsb // 4,))
        for nbytes, ptr in ((wsb - 1, ws.t.data_ptr()), (wsb, None)):
            c.y.t.fill_(SENTINEL)
            rc = lib.rg_f32p_conv(0, c.x.t.data_ptr(), c.w.t.data_ptr(), c.y.t.data_ptr(), *dims, products, None, None, 1.0, ptr, nbytes, E.stream)
            torch.cuda.synchronize()
            assert rc == RG_EWORKSPACE and bool((bits(c.y.t) == SBITS).all()) and bool((bits(ws.flat) == SBITS).all())
        for null in (0, 1, 2):
            args = [c.x.t.data_ptr(), c.w.t.data_ptr(), c.y.t.data_ptr()]
            args[null] = None
            assert lib.rg_f32p_conv(0, *args, *dims, products, None, None, 1.0, ws.t.data_ptr(), wsb, E.stream) == RG_EINVAL
        assert lib.rg_f32p_conv(0, c.x.t.data_ptr(), c.w.t.data_ptr(), c.y.t.data_ptr(), 1, 8, 16, 256, 64, products, None, None, 1.0,
                                ws.t.data_ptr(), wsb, E.stream) == RG_EUNSUPPORTED
    wd = (1, 16, 16, 256, 16)
    A, B, dw0 = R.wgrad_operands(wd, False)
    lo, hi = _operand(A[0]), _operand(B[0])
    for products in (6, 3):
        with _Options(lib, wgrad8_blocks=8):
            assert int(lib.rg_f32p_wgrad_workspace_bytes(*wd, products, 0)) > 0
            dw = _wgrad(E, wd, products, [lo], [hi], None, 0, expect=RG_EWORKSPACE, short=1)
            assert bool((bits(dw) == SBITS).all())
        dw = _out((256, 4, 4, 16))
        for l1, h1 in ((lo.t.data_ptr(), None), (None, hi.t.data_ptr())):
            rc = lib.rg_f32p_wgrad(lo.t.data_ptr(), hi.t.data_ptr(), l1, h1, dw.t.data_ptr(), *wd, products, 0, None, 0, E.stream)
            torch.cuda.synchronize()
            assert rc == RG_EINVAL and bool((bits(dw.t) == SBITS).all())
        assert lib.rg_f32p_wgrad(lo.t.data_ptr(), hi.t.data_ptr(), None, None, dw.t.data_ptr(), 1, 8, 16, 256, 16, products, 0, None, 0,
                                 E.stream) == RG_EUNSUPPORTED


# ------------------------------------------------------------------ (g) through HipOps: real splits, Gaussian operands, fp64
TOL = {6: 2e-6, 3: 6e-5}                             # of max|ref| (tests/test_f32_planes_gpu.py); 1e-4 for the column sums


def _ops(products, monkeypatch):
    from rna_gan_amd.ops_hip import HipOps
    monkeypatch.setenv("RNAGAN_F32_PLANES", str(products))
    return HipOps(torch.float32, DEV)


def _cw(w):
    from rna_gan_amd.engine import ConvW
    return ConvW(w.contiguous(), None, torch.zeros_like(w), None, "OHWI")


def _err(name, dims, products, got, ref, tol, scale=None):
    scale = float(ref.abs().max()) if scale is None else scale
    e = float((got.double() - ref).abs().max()) / scale
    print("ERR %s %s %d %.3e" % (name, R.case_id(dims), products, e))
    assert e <= tol, "%s %s: max|err| / max|ref| = %.3e > %.1e" % (name, dims, e, tol)


def _stats_err(name, dims, products, st, ref):
    C = ref.shape[-1]
    r = ref.reshape(-1, C)
    s = st.double().sum(0)
    e1 = float((s[0] - r.sum(0)).abs().max()) / float(r.abs().sum(0).max())
    e2 = float((s[1] - (r * r).sum(0)).abs().max()) / float((r * r).sum(0).max())
    print("ERR %s.sum %s %d %.3e" % (name, R.case_id(dims), products, e1))
    print("ERR %s.sumsq %s %d %.3e" % (name, R.case_id(dims), products, e2))
    assert e1 <= 1e-4 and e2 <= 1e-4


HIPOPS_CASES = [("down", (5, 8, 8, 256, 64), False), ("down", (3, 16, 16, 128, 64), False), ("up", (5, 8, 8, 64, 256), False),
                ("up", (3, 16, 16, 64, 128), False), ("up", (5, 8, 8, 64, 64), False), ("wgrad", (5, 8, 8, 256, 16), False),
                ("wgrad", (5, 8, 8, 128, 32), False), ("down", R.UNSPLIT["down256"], True), ("up", R.UNSPLIT["up256"], True)]


@pytest.mark.parametrize("products", [6, 3])
@pytest.mark.parametrize("op,dims,stats", HIPOPS_CASES, ids=R.case_id)
def test_hipops_gaussian_against_fp64(op, dims, stats, products, monkeypatch):
    ops = _ops(products, monkeypatch)
    N, Hl, Wl, O, I = dims
    sa, sb, _ = R.operand_shapes(op, *dims)
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(sa, generator=gen).to(DEV)
    b = (torch.randn(sb, generator=gen) * (0.05 if op != "wgrad" else 1.0)).to(DEV)
    up = 1 if op == "up" else 0
    if op == "wgrad":
        assert ops.lib.rg_f32p_wgrad_supported(*dims, products) == 1
        cw = _cw(torch.zeros(O, 4, 4, I, device=DEV))
        ops.conv_wgrad(a, b, cw, False)
        ref = ref_wgrad(a.double(), b.double())
        _err("conv_wgrad", dims, products, cw.dw, ref, TOL[products])
        ops.conv_wgrad2(a, b, a, b, cw, True)
        _err("conv_wgrad2.acc", dims, products, cw.dw, 3 * ref, 2 * TOL[products])
        return
    assert ops.lib.rg_f32p_conv_supported(up, *dims, products) == 1
    rows = int(ops.lib.rg_f32p_conv_stats_rows(up, *dims, products))
    assert (rows > 0) == stats or (up and O == 64 and products == 3 and I % 128 == 0)
    ref = (ref_up if up else ref_down)(a.double(), b.double())
    run = ops.conv_up if up else ops.conv_down
    y, st = run(a, _cw(b), want_stats=True)
    _err("conv_" + op, dims, products, y, ref, TOL[products])
    if rows > 0:
        assert st is not None and st.shape[0] == rows          # BatchNorm column sums from the epilogue (unsplit launches)
        _stats_err("conv_" + op, dims, products, st, ref)
    else:
        assert st is None
    if up:                                                     # with the consumer's LeakyReLU backward (fused into the 64-column kernel)
        a0 = torch.randn(ref.shape, generator=gen).to(DEV)
        gm = ops.conv_up(a, _cw(b), a0, 0.2)
        _err("conv_up.masked", dims, products, gm, ref * torch.where(a0 > 0, 1.0, 0.2).double(), TOL[products], scale=float(ref.abs().max()))
