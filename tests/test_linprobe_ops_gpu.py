"""rg_linear_scores_f64, rg_softmax_residual_f64 and rg_rows_weighted_colsums_f64 (include/rnagan_hip.h,
rna_gan_amd/csrc/rg_linprobe.hip) op by op through ctypes, on both builds of the library, against the numpy restatements of
tests/linprobe_refs.py (pinned without a GPU by tests/test_linprobe_refs_cpu.py).

Operands live inside NaN-filled allocations (a row or column read past the operand shows as a NaN; such reads stay inside the
allocation, so nothing can fault); outputs and the workspace live inside allocations pre-filled with one pattern: what is outside
them -- the columns C .. ldz of a row of z included -- must keep it.

Scores and column sums: the contract is a CHAIN of fma in a stated order, so the device must EQUAL the restatement bit for bit on
arbitrary normal floats (the fma rounds at every step: its order, and whether it is an fma at all, shows).  n in {1, 63, 64, 65,
255, 256, 257, 600} covers the 32-row tile of the scores, the 256-row block of the column sums and three blocks with a ragged
last one; C in {1, 2, 3, 17, 64, 65} the 8-class chunk of both kernels, one class, and chunks with a ragged last one;
F in {1, 31, 32, 33, 100} the 64-column workgroup of the column sums and a single, partly filled staging pass of the scores.
Every n meets every F; the C values rotate over them, so every (F, C) pair and five of the six class counts per n turn up.
The scores kernel stages 256 features per pass: F in {255, 256, 257, 600} (test_scores_more_than_one_staging_pass) takes it
through a full pass, the restaging behind the trailing barrier, a second pass of one feature and a ragged third one -- the
path of the production width F = 2 048 -- and gives n = 1, 65 and 257 the class count the rotation leaves out.

rg_softmax_residual_f64 uses the device's exp and log: bounded, not exact.  The reference is the restatement in np.longdouble.
The bound counts roundings to first order, u = 2^-53, with the device's exp and log taken at 2 ulp each -- the HIP math
documentation is not among the files at hand, so this is ASSUMED (the public table states 1 ulp for both); 1 ulp <= 2 u relative:
  d_c = z_c - m           one rounded subtraction: d_c (1 + delta), |delta| <= u, which exp turns into a relative |d_c| u
  e_c = exp(d_c)          relative tau_c = (|d_c| + 2 * 2) u
  s = sum e_c             C - 1 additions of positive terms: relative sigma = sum_c p_c tau_c + (C - 1) u
  p_c = e_c / s           relative tau_c + sigma + u
  resid = wt (p_c - [c == y])   |wt| (p_c (tau_c + sigma + u) + u |p_c - [c == y]|) + u |resid|, + |wt| 2^-1022 for an e_c that
                          leaves the normal range
  loss = wt (log(s) - d_y)      |wt| (sigma + 2 * 2 u |log s| + u |d_y| + u |log s - d_y|) + u |loss|
The whole is multiplied by 1.001 for the second-order terms.  The worst observed multiple of the bound is printed (the record
is profiles/linprobe_op_errors.txt; the bound, not the record, is the gate)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from guarded import DEV
from linprobe_refs import U, colsums_ref, scores_ref, softmax_residual_ref
from test_kid_ops_gpu import DSENT, GuardedD, Rows, _same_bits
from test_repr_ops_gpu import Ints, RowsD

BUILDS = ["bf16", "f16"]
ROW_COUNTS = [1, 63, 64, 65, 255, 256, 257, 600]
F_SIZES = [1, 31, 32, 33, 100]
CLASSES = [1, 2, 3, 17, 64, 65]
STRIDES = ((0, 0, 0), (5, 3, 0), (0, 0, 1), (5, 3, 3))       # (ldx - F, ldz / ldr - C, elements the base pointers are off 256 bytes)
EINVAL, EWORKSPACE = -1, -3
EXP_ULP = LOG_ULP = 2.0
TINY = float(np.finfo(np.float64).tiny)


def _shapes(F):
    """every n for this F, the class counts rotating: over the five F every (F, C) pair turns up and every n meets five of the six
    class counts (the sixth is MISSING_C[n], which test_scores_more_than_one_staging_pass uses)"""
    j = F_SIZES.index(F) if F in F_SIZES else 0
    return [(n, CLASSES[(i + j) % len(CLASSES)]) for i, n in enumerate(ROW_COUNTS)]


MISSING_C = {n: CLASSES[(i + len(F_SIZES)) % len(CLASSES)] for i, n in enumerate(ROW_COUNTS)}
MULTI_PASS_F = [255, 256, 257, 600]                          # around one staging pass of 256 features, and over two with a ragged third

_CASES = {}


def _case(n, F, C):
    """arbitrary normal floats and the restatements' results, computed once and shared by the builds and the tests"""
    key = (n, F, C)
    if key not in _CASES:
        rng = np.random.default_rng([n, F, C])
        x = rng.standard_normal((n, F)).astype(np.float32)
        w, bias, r = rng.standard_normal((C, F)), rng.standard_normal(C), rng.standard_normal((n, C))
        z0 = scores_ref(x, w, None)
        _CASES[key] = dict(x=x, w=w, bias=bias, r=r, z=z0 + bias[None, :], z0=z0, s1=colsums_ref(x, r, 1), s2=colsums_ref(x, r, 2))
    return _CASES[key]


def _scores(lib, x, w, bias, ldx_extra=0, ldz_extra=0, shift=0):
    n, F = x.shape
    C = w.shape[0]
    dx, dw = Rows(x, F + ldx_extra, shift), RowsD(w, F + ldx_extra, shift)
    db = None if bias is None else RowsD(bias[None, :], C, shift)
    ldz = C + ldz_extra
    z = GuardedD((n, ldz))
    rc = lib.rg_linear_scores_f64(dx.ptr, dx.ld, n, F, dw.ptr, dw.ld, C, None if db is None else db.ptr, z.t.data_ptr(), ldz, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert z.intact(), "rg_linear_scores_f64 wrote outside z"
    assert bool((z.t[:, C:] == DSENT).all()), "rg_linear_scores_f64 wrote the columns past C of a row of z"
    return z.t[:, :C].cpu().numpy()


def _colsums(lib, x, r, power, ldx_extra=0, ldr_extra=0, shift=0, ws_extra=0):
    n, F = x.shape
    C = r.shape[1]
    dx, dr = Rows(x, F + ldx_extra, shift), RowsD(r, C + ldr_extra, shift)
    need = lib.rg_colsums_ws_bytes(n, F, C)
    assert need == 8 * ((n + 255) // 256) * C * F
    ws, out = GuardedD((need // 8 + ws_extra,)), GuardedD((C, F))
    rc = lib.rg_rows_weighted_colsums_f64(dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, power, ws.t.data_ptr(), need, out.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert out.intact() and ws.intact(), "rg_rows_weighted_colsums_f64 wrote outside out / the workspace"
    assert ws_extra == 0 or bool((ws.t[need // 8:] == DSENT).all()), "more of the workspace was written than its stated size"
    return out.t.cpu().numpy()


# ------------------------------------------------------------------ rg_linear_scores_f64
@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_scores_equal_the_fma_chain(half, F):
    lib = _abi.load(half)
    for n, C in _shapes(F):
        ref = _case(n, F, C)
        got = _scores(lib, ref["x"], ref["w"], ref["bias"])
        assert np.isfinite(got).all(), "%s n=%d F=%d C=%d: a row, class or column past the operands was read" % (half, n, F, C)
        assert _same_bits(got, ref["z"]), "%s n=%d F=%d C=%d: z differs from the chain" % (half, n, F, C)
        assert _same_bits(_scores(lib, ref["x"], ref["w"], None), ref["z0"]), "%s n=%d F=%d C=%d: bias = NULL" % (half, n, F, C)
    if F >= 31:                                               # the operands can tell: the same chain with a rounded product gives other bits
        ref = _case(600, F, _shapes(F)[-1][1])
        xd, acc = ref["x"].astype(np.float64), 0.0
        for f in range(F):
            acc = acc + xd[:, f:f + 1] * ref["w"][None, :, f]
        assert not _same_bits(ref["z0"], acc) and np.allclose(ref["z0"], acc, rtol=0, atol=1e-9)


@pytest.mark.parametrize("half", BUILDS)
def test_scores_strides_and_alignment(half):
    lib = _abi.load(half)
    for n, F, C in ((65, 33, 3), (257, 100, 17), (33, 70, 9)):
        ref = _case(n, F, C)
        for ldx_extra, ldz_extra, shift in STRIDES:
            got = _scores(lib, ref["x"], ref["w"], ref["bias"], ldx_extra, ldz_extra, shift)
            assert _same_bits(got, ref["z"]), "%s n=%d F=%d C=%d ld +%d +%d shift %d" % (half, n, F, C, ldx_extra, ldz_extra, shift)


_MULTI = {}


def _multi_case(n, F, C):
    """as _case without the column sums (their kernel has no feature pass; a 600-column restatement would only cost time)"""
    key = (n, F, C)
    if key not in _MULTI:
        rng = np.random.default_rng([n, F, C, 1])
        x, w, bias = rng.standard_normal((n, F)).astype(np.float32), rng.standard_normal((C, F)), rng.standard_normal(C)
        z0 = scores_ref(x, w, None)
        _MULTI[key] = dict(x=x, w=w, bias=bias, z0=z0, z=z0 + bias[None, :])
    return _MULTI[key]


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", MULTI_PASS_F)
def test_scores_more_than_one_staging_pass(half, F):
    """F = 255: one pass, one feature short; 256: exactly one; 257: a second pass of ONE feature behind the barrier; 600: two full
    passes and a ragged third.  Both bias modes, every stride / alignment variant, the row tails around the 32-row tile."""
    lib = _abi.load(half)
    for n in (1, 33, 65) if F != 600 else (33, 257):
        ref = _multi_case(n, F, MISSING_C[n] if n in MISSING_C else 9)
        for ldx_extra, ldz_extra, shift in STRIDES:
            what = "%s n=%d F=%d C=%d ld +%d +%d shift %d" % (half, n, F, ref["w"].shape[0], ldx_extra, ldz_extra, shift)
            got = _scores(lib, ref["x"], ref["w"], ref["bias"], ldx_extra, ldz_extra, shift)
            assert np.isfinite(got).all(), what + ": a row, class or column past the operands was read"
            assert _same_bits(got, ref["z"]), what + ": z differs from the chain"
            assert _same_bits(_scores(lib, ref["x"], ref["w"], None, ldx_extra, ldz_extra, shift), ref["z0"]), what + ": bias = NULL"
    ref = _multi_case(33, F, 9)                               # the operands can tell a rounded product from the fma
    xd, acc = ref["x"].astype(np.float64), 0.0
    for f in range(F):
        acc = acc + xd[:, f:f + 1] * ref["w"][None, :, f]
    assert not _same_bits(ref["z0"], acc) and np.allclose(ref["z0"], acc, rtol=0, atol=1e-9)


# ------------------------------------------------------------------ rg_rows_weighted_colsums_f64
@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_colsums_equal_the_blocked_chain(half, F):
    lib = _abi.load(half)
    for n, C in _shapes(F):
        ref = _case(n, F, C)
        for power in (1, 2):
            got = _colsums(lib, ref["x"], ref["r"], power, ws_extra=64)
            assert np.isfinite(got).all(), "%s n=%d F=%d C=%d: a row or column past the operands was read" % (half, n, F, C)
            assert _same_bits(got, ref["s%d" % power]), "%s n=%d F=%d C=%d power %d" % (half, n, F, C, power)
    if F >= 31:                                               # the operands can tell the blocked chain from another order
        ref = _case(600, F, _shapes(F)[-1][1])
        xd, plain = ref["x"].astype(np.float64), 0.0
        for row in range(600):                                # one chain over all rows, the product rounded
            plain = plain + ref["r"][row][:, None] * xd[row][None, :]
        assert not _same_bits(ref["s1"], plain) and np.allclose(ref["s1"], plain, rtol=0, atol=1e-9)


@pytest.mark.parametrize("half", BUILDS)
def test_colsums_strides_alignment_and_the_column_of_ones(half):
    lib = _abi.load(half)
    for n, F, C in ((65, 33, 3), (257, 100, 17), (600, 70, 9)):
        ref = _case(n, F, C)
        for ldx_extra, ldr_extra, shift in STRIDES:
            for power in (1, 2):
                got = _colsums(lib, ref["x"], ref["r"], power, ldx_extra, ldr_extra, shift)
                assert _same_bits(got, ref["s%d" % power]), "%s n=%d F=%d C=%d ld +%d +%d shift %d power %d" % (
                    half, n, F, C, ldx_extra, ldr_extra, shift, power)
    # the two other uses: r a 0/1 column gives the sums and sums of squares of the selected rows; x a column of ones gives the
    # column sums of r -- the same blocked order
    ref = _case(600, 33, 3)
    mask = (np.arange(600) % 3 != 0).astype(np.float64)[:, None]
    for power in (1, 2):
        assert _same_bits(_colsums(lib, ref["x"], mask, power), colsums_ref(ref["x"], mask, power))
    ones = np.ones((600, 1), dtype=np.float32)
    assert _same_bits(_colsums(lib, ones, ref["r"], 1), colsums_ref(ones, ref["r"], 1))
    # exact zeros in r (masked rows) leave the sums of the other rows as they are
    r0 = ref["r"] * mask
    assert _same_bits(_colsums(lib, ref["x"], r0, 1), colsums_ref(ref["x"], r0, 1))


# ------------------------------------------------------------------ rg_softmax_residual_f64
def _residual_bounds(z, label, weight):
    """(resid, loss) of the longdouble restatement and the two bounds of the module docstring, as longdouble arrays"""
    L = np.longdouble
    n, C = z.shape
    old = np.seterr(all="ignore")                            # the masked rows hold NaN logits
    resid, loss = softmax_residual_ref(z, label, weight, L)
    zl = z.astype(L)
    wt = np.abs(np.ones(n) if weight is None else weight).astype(L)
    d = zl - zl.max(axis=1)[:, None]
    e = np.exp(d)
    s = e.sum(axis=1)
    p = e / s[:, None]
    ok = (label >= 0) & (label < C)
    y = np.where(ok, label, 0)
    onehot = (np.arange(C)[None, :] == y[:, None]).astype(L)
    tau = (np.abs(d) + 2.0 * EXP_ULP) * U
    sigma = (p * tau).sum(axis=1) + (C - 1) * U
    b_resid = wt[:, None] * (p * (tau + sigma[:, None] + U) + U * np.abs(p - onehot) + TINY) + U * np.abs(resid)
    dy, ls = d[np.arange(n), y], np.log(s)
    b_loss = wt * (sigma + 2.0 * LOG_ULP * U * np.abs(ls) + U * np.abs(dy) + U * np.abs(ls - dy)) + U * np.abs(loss)
    b_resid[~ok], b_loss[~ok] = 0, 0                         # masked rows: exact zeros
    np.seterr(**old)
    return resid, loss, 1.001 * b_resid, 1.001 * b_loss


def _residual(lib, z, label, weight, ldz_extra=0, ldr_extra=0, shift=0):
    n, C = z.shape
    dz, dl = RowsD(z, C + ldz_extra, shift), Ints(label, 0)  # a label read past the end would be a valid class 0
    dw = None if weight is None else RowsD(weight[None, :], n, shift)
    ldr = C + ldr_extra
    resid, loss = GuardedD((n, ldr)), GuardedD((n,))
    rc = lib.rg_softmax_residual_f64(dz.ptr, dz.ld, n, C, dl.ptr, None if dw is None else dw.ptr, resid.t.data_ptr(), ldr,
                                     loss.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert resid.intact() and loss.intact(), "rg_softmax_residual_f64 wrote outside resid / row_loss"
    assert bool((resid.t[:, C:] == DSENT).all()), "rg_softmax_residual_f64 wrote the columns past C of a row of resid"
    return resid.t[:, :C].cpu().numpy(), loss.t.cpu().numpy()


def _logits(n, C, seed):
    rng = np.random.default_rng([seed, n, C])
    z = rng.standard_normal((n, C)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))
    label = rng.integers(0, C, size=n).astype(np.int32)
    label[::7] = -1                                          # masked rows: both sides of [0, C), their logits NaN
    label[3::11] = C
    z[(label < 0) | (label >= C)] = np.nan
    if n > 8 and C > 1:                                       # +-1000: exp underflows, never overflows
        z[1] = 1000.0 * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
        z[2] = -1000.0
        z[2, C - 1] = 1000.0
        label[1], label[2] = 1, 0
    return z, label, rng.uniform(0.25, 4.0, size=n)


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("C", CLASSES)
def test_residual_and_loss_within_the_rounding_bound(half, C):
    lib = _abi.load(half)
    worst = 0.0
    for n in ROW_COUNTS:
        z, label, wt = _logits(n, C, 1)
        for weight in (None, wt):
            want_r, want_l, b_r, b_l = _residual_bounds(z, label, weight)
            got_r, got_l = _residual(lib, z, label, weight)
            masked = (label < 0) | (label >= C)
            assert not got_r[masked].any() and not got_l[masked].any(), "a masked row must be exact zeros"
            assert not np.signbit(got_r[masked]).any() and not np.signbit(got_l[masked]).any()
            assert np.isfinite(got_r).all() and np.isfinite(got_l).all(), "logits of +-1000 must give finite results"
            err_r, err_l = np.abs(got_r.astype(np.longdouble) - want_r), np.abs(got_l.astype(np.longdouble) - want_l)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = max(float(np.nanmax(np.where(b_r > 0, err_r / b_r, 0))), float(np.nanmax(np.where(b_l > 0, err_l / b_l, 0))))
            worst = max(worst, ratio)
            assert np.all(err_r <= b_r) and np.all(err_l <= b_l), "%s n=%d C=%d: %.3g of the bound" % (half, n, C, ratio)
            if n > 8 and C > 1:
                assert got_l[2] == 2000.0 * (1.0 if weight is None else wt[2]) and got_r[2, 0] == -(1.0 if weight is None else wt[2])
    print("%s C=%d: worst |device - longdouble| / bound = %.3f" % (half, C, worst))


@pytest.mark.parametrize("half", BUILDS)
def test_residual_strides_and_a_nan_row(half):
    lib = _abi.load(half)
    for n, C in ((65, 3), (257, 17), (600, 2)):
        z, label, wt = _logits(n, C, 2)
        base = _residual(lib, z, label, wt)
        for _, ld_extra, shift in STRIDES[1:]:
            got = _residual(lib, z, label, wt, ld_extra, ld_extra + 1, shift)
            assert _same_bits(got[0], base[0]) and _same_bits(got[1], base[1]), "the values must not depend on strides or alignment"
        z2 = z.copy()
        r = 5
        assert 0 <= label[r] < C
        z2[r, C - 1] = np.nan                                 # one NaN logit: its row is NaN, no other row changes
        got = _residual(lib, z2, label, wt)
        assert np.isnan(got[0][r]).all() and np.isnan(got[1][r])
        keep = np.arange(n) != r
        assert _same_bits(got[0][keep], base[0][keep]) and _same_bits(got[1][keep], base[1][keep])


# ------------------------------------------------------------------ all three: replay, rejected arguments
@pytest.mark.parametrize("half", BUILDS)
def test_graph_replay_gives_the_bits_of_the_eager_calls(half):
    lib = _abi.load(half)
    n, F, C = 257, 33, 3
    ref = _case(n, F, C)
    label = (np.arange(n) % (C + 1) - 1).astype(np.int32)
    eager_r, eager_l = _residual(lib, ref["z"], label, None)
    eager_g = _colsums(lib, ref["x"], eager_r, 1)
    dx, dw, db, dl = Rows(ref["x"], F + 5, 1), RowsD(ref["w"], F), RowsD(ref["bias"][None, :], C), Ints(label, 0)
    need = lib.rg_colsums_ws_bytes(n, F, C)
    z, resid, loss, ws, out = GuardedD((n, C)), GuardedD((n, C)), GuardedD((n,)), GuardedD((need // 8,)), GuardedD((C, F))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.rg_linear_scores_f64(dx.ptr, dx.ld, n, F, dw.ptr, dw.ld, C, db.ptr, z.t.data_ptr(), C, st) == 0, lib.rg_last_error()
        assert lib.rg_softmax_residual_f64(z.t.data_ptr(), C, n, C, dl.ptr, None, resid.t.data_ptr(), C, loss.t.data_ptr(), st) == 0, \
            lib.rg_last_error()
        assert lib.rg_rows_weighted_colsums_f64(dx.ptr, dx.ld, n, F, resid.t.data_ptr(), C, C, 1, ws.t.data_ptr(), need,
                                                out.t.data_ptr(), st) == 0, lib.rg_last_error()
    for g in (z, resid, loss, out):
        g.t.fill_(DSENT)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(z.t.cpu().numpy(), ref["z"])
    assert _same_bits(resid.t.cpu().numpy(), eager_r) and _same_bits(loss.t.cpu().numpy(), eager_l)
    assert _same_bits(out.t.cpu().numpy(), eager_g)
    assert all(g.intact() for g in (z, resid, loss, ws, out))


@pytest.mark.parametrize("half", BUILDS)
def test_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    n, F, C = 70, 17, 5
    ref = _case(n, F, C)
    dx, dw, db = Rows(ref["x"], F + 3), RowsD(ref["w"], F + 2), RowsD(ref["bias"][None, :], C)
    dz, dr, dl, dwt = RowsD(ref["z"], C + 1), RowsD(ref["r"], C + 1), Ints(np.arange(n) % C, 0), RowsD(np.ones((1, n)), n)
    need = lib.rg_colsums_ws_bytes(n, F, C)
    z, resid, loss, ws, out = GuardedD((n, C)), GuardedD((n, C)), GuardedD((n,)), GuardedD((need // 8,)), GuardedD((C, F))
    outputs = (z, resid, loss, ws, out)
    pz, pr, pl, pw, po = (g.t.data_ptr() for g in outputs)

    def check(name, rc, want, what):
        assert rc == want, "%s, %s: returned %d" % (name, what, rc)
        assert name[3:].encode() in lib.rg_last_error(), what
        torch.cuda.synchronize()
        assert all(g.untouched() for g in outputs), "%s, %s: something was written" % (name, what)

    #                x       ldx    n  F  w       ldw    C  bias    z   ldz
    bad = {"F = 0": (dx.ptr, dx.ld, n, 0, dw.ptr, dw.ld, C, db.ptr, pz, C),
           "C = 0": (dx.ptr, dx.ld, n, F, dw.ptr, dw.ld, 0, db.ptr, pz, C),
           "n < 0": (dx.ptr, dx.ld, -1, F, dw.ptr, dw.ld, C, db.ptr, pz, C),
           "ldx < F": (dx.ptr, F - 1, n, F, dw.ptr, dw.ld, C, db.ptr, pz, C),
           "ldw < F": (dx.ptr, dx.ld, n, F, dw.ptr, F - 1, C, db.ptr, pz, C),
           "ldz < C": (dx.ptr, dx.ld, n, F, dw.ptr, dw.ld, C, db.ptr, pz, C - 1),
           "x = NULL": (None, dx.ld, n, F, dw.ptr, dw.ld, C, db.ptr, pz, C),
           "w = NULL": (dx.ptr, dx.ld, n, F, None, dw.ld, C, db.ptr, pz, C),
           "z = NULL": (dx.ptr, dx.ld, n, F, dw.ptr, dw.ld, C, db.ptr, None, C)}
    for what, args in bad.items():
        check("rg_linear_scores_f64", lib.rg_linear_scores_f64(*args, None), EINVAL, what)
    #                z       ldz    n  C  label   weight   resid ldr row_loss
    bad = {"C = 0": (dz.ptr, dz.ld, n, 0, dl.ptr, dwt.ptr, pr, C, pl),
           "n < 0": (dz.ptr, dz.ld, -1, C, dl.ptr, dwt.ptr, pr, C, pl),
           "ldz < C": (dz.ptr, C - 1, n, C, dl.ptr, dwt.ptr, pr, C, pl),
           "ldr < C": (dz.ptr, dz.ld, n, C, dl.ptr, dwt.ptr, pr, C - 1, pl),
           "z = NULL": (None, dz.ld, n, C, dl.ptr, dwt.ptr, pr, C, pl),
           "label = NULL": (dz.ptr, dz.ld, n, C, None, dwt.ptr, pr, C, pl),
           "resid = NULL": (dz.ptr, dz.ld, n, C, dl.ptr, dwt.ptr, None, C, pl),
           "row_loss = NULL": (dz.ptr, dz.ld, n, C, dl.ptr, dwt.ptr, pr, C, None)}
    for what, args in bad.items():
        check("rg_softmax_residual_f64", lib.rg_softmax_residual_f64(*args, None), EINVAL, what)
    #                x       ldx    n  F  r       ldr    C  power ws  bytes  out  code
    bad = {"F = 0": (dx.ptr, dx.ld, n, 0, dr.ptr, dr.ld, C, 1, pw, need, po, EINVAL),
           "C = 0": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, 0, 1, pw, need, po, EINVAL),
           "n < 0": (dx.ptr, dx.ld, -1, F, dr.ptr, dr.ld, C, 1, pw, need, po, EINVAL),
           "ldx < F": (dx.ptr, F - 1, n, F, dr.ptr, dr.ld, C, 1, pw, need, po, EINVAL),
           "ldr < C": (dx.ptr, dx.ld, n, F, dr.ptr, C - 1, C, 1, pw, need, po, EINVAL),
           "power = 0": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 0, pw, need, po, EINVAL),
           "power = 3": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 3, pw, need, po, EINVAL),
           "x = NULL": (None, dx.ld, n, F, dr.ptr, dr.ld, C, 1, pw, need, po, EINVAL),
           "r = NULL": (dx.ptr, dx.ld, n, F, None, dr.ld, C, 1, pw, need, po, EINVAL),
           "ws = NULL": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 1, None, need, po, EINVAL),
           "out = NULL": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 1, pw, need, None, EINVAL),
           "ws one byte short": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 1, pw, need - 1, po, EWORKSPACE),
           "ws misaligned": (dx.ptr, dx.ld, n, F, dr.ptr, dr.ld, C, 1, pw + 4, need, po, EWORKSPACE)}
    for what, args in bad.items():
        check("rg_rows_weighted_colsums_f64", lib.rg_rows_weighted_colsums_f64(*args[:-1], None), args[-1], what)
    assert lib.rg_colsums_ws_bytes(-1, F, C) == 0 and lib.rg_colsums_ws_bytes(n, 0, C) == 0 and lib.rg_colsums_ws_bytes(n, F, 0) == 0
    assert lib.rg_colsums_ws_bytes(0, F, C) == 0 and lib.rg_colsums_ws_bytes(257, F, C) == 2 * C * F * 8
    # no rows.  Scores and residual: RG_OK, nothing launched.  Column sums: out is WRITTEN as the empty sums (+0.0), x, r and the
    # workspace are not looked at (NULL, misaligned and too short are all accepted), a NULL out is still refused
    assert lib.rg_linear_scores_f64(dx.ptr, dx.ld, 0, F, dw.ptr, dw.ld, C, db.ptr, pz, C, None) == 0
    assert lib.rg_softmax_residual_f64(dz.ptr, dz.ld, 0, C, dl.ptr, None, pr, C, pl, None) == 0
    check("rg_rows_weighted_colsums_f64", lib.rg_rows_weighted_colsums_f64(dx.ptr, dx.ld, 0, F, dr.ptr, dr.ld, C, 1, pw, need, None, None),
          EINVAL, "out = NULL without rows")
    for power, args in ((1, (dx.ptr, dx.ld, 0, F, dr.ptr, dr.ld, C, 1, pw, need, po)), (2, (None, dx.ld, 0, F, None, dr.ld, C, 2, None, 0, po)),
                        (1, (dx.ptr, dx.ld, 0, F, dr.ptr, dr.ld, C, 1, pw + 4, 3, po))):
        out.t.fill_(DSENT)
        assert lib.rg_rows_weighted_colsums_f64(*args, None) == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        got = out.t.cpu().numpy()
        assert not got.any() and not np.signbit(got).any(), "no rows: out must be +0.0 everywhere"
        assert out.intact() and all(g.untouched() for g in (z, resid, loss, ws))
