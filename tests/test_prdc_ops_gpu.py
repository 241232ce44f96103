"""rg_knn_radii2, rg_radius_hits and rg_pairdist_ws_bytes (include/rnagan_hip.h, rna_gan_amd/csrc/rg_knn.hip) op by op through
ctypes, on both builds of the library, against the numpy restatement of tests/prdc_refs.py (pinned without a GPU by
tests/test_prdc_refs_cpu.py).

Operands live inside NaN-filled allocations (a row or column read past the operand shows as a NaN distance, which never hits and
turns a radius or a minimum into +inf; such reads stay inside the allocation, so nothing can fault).  Outputs and the workspace
live inside allocations pre-filled with one pattern: what is outside them must keep it, and the workspace handed over is EXACTLY
rg_pairdist_ws_bytes(...) long in every call.

Exact cases: integer features in [-3, 3].  Every d2 is an exact integer in fp64 whatever the order or the fusing, so radii,
counts and minima must EQUAL the restatement, with the ties and the planted duplicates of prdc_refs.integer_case.  Row counts
around the 64-row tile (2, 63, 64, 65) and over three tiles with a ragged last one (130), in every na x nb combination for the
hits; feature counts around the 32-feature staging pass (1, 31, 32, 33), over three passes (70) and eight (256).

General floats: device and restatement are each within GAMMA(F) of the exact d2 (prdc_refs.GAMMA: at most F + 2 roundings of
non-negative terms), order statistics and minima are monotone in the entries: |dev - ref| <= 2 GAMMA max(dev, ref) for radii
and minima, and count_strict <= count_dev <= count_loose with the restatement's counts at d2 (1 + 2 GAMMA) and d2 (1 - 2 GAMMA)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from guarded import DEV, SBITS
from prdc_refs import GAMMA, dist2, hits_ref, integer_case, radii2_ref
from test_kid_ops_gpu import DSENT, GuardedD, Rows, _same_bits

BUILDS = ["bf16", "f16"]
ROW_COUNTS = [2, 63, 64, 65, 130]
F_SIZES = [1, 31, 32, 33, 70, 256]
STRIDES = ((0, 0), (5, 0), (0, 1), (5, 3))                  # (lda - F, floats the base pointer is off a 256-byte boundary)
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
WS_BYTE = 0xA5


class GuardedI:
    """n int32 in the middle of an allocation filled with SBITS, the n themselves included"""

    def __init__(self, n, pad=512):
        self.flat = torch.full((pad + n + pad,), SBITS, dtype=torch.int32, device=DEV)
        self.t, self.pad, self.n = self.flat[pad:pad + n], pad, n

    def intact(self):
        return bool((self.flat[:self.pad] == SBITS).all()) and bool((self.flat[self.pad + self.n:] == SBITS).all())

    def untouched(self):
        return bool((self.flat == SBITS).all())


class GuardedWS:
    """nbytes of workspace (8-byte aligned) in the middle of an allocation filled with WS_BYTE"""

    def __init__(self, nbytes, pad=4096):
        self.flat = torch.full((pad + nbytes + pad,), WS_BYTE, dtype=torch.uint8, device=DEV)
        self.ptr, self.pad, self.n = self.flat.data_ptr() + pad, pad, nbytes
        assert self.ptr % 8 == 0

    def intact(self):
        return bool((self.flat[:self.pad] == WS_BYTE).all()) and bool((self.flat[self.pad + self.n:] == WS_BYTE).all())

    def untouched(self):
        return bool((self.flat == WS_BYTE).all())


class Radii:
    """the (nb,) fp64 radii operand inside an allocation filled with +inf: a radius read past the end would hit everything"""

    def __init__(self, r):
        self.flat = torch.full((256 + len(r) + 256,), float("inf"), dtype=torch.float64, device=DEV)
        self.flat[256:256 + len(r)] = torch.from_numpy(np.asarray(r, dtype=np.float64)).to(DEV)
        self.ptr = self.flat.data_ptr() + 256 * 8


def _knn(lib, a, k):
    """one rg_knn_radii2 call -> r2 as numpy fp64; the return code, the guards of r2 and of an exactly sized workspace checked"""
    need = lib.rg_pairdist_ws_bytes(a.n, a.n, k)
    assert need == ((a.n + 63) // 64) * a.n * k * 8
    ws, r2 = GuardedWS(need), GuardedD((a.n,))
    rc = lib.rg_knn_radii2(a.ptr, a.ld, a.n, a.F, k, ws.ptr, need, r2.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert r2.intact() and ws.intact(), "rg_knn_radii2 wrote outside r2 / the stated workspace bytes"
    return r2.t.cpu().numpy()


def _hits(lib, a, b, rb2):
    """one rg_radius_hits call -> (count or None, mind2) as numpy; rb2: numpy radii or None (the minimum-only form)"""
    need = lib.rg_pairdist_ws_bytes(a.n, b.n, 0)
    assert need == ((b.n + 63) // 64) * a.n * 12
    ws, mind2 = GuardedWS(need), GuardedD((a.n,))
    count = None if rb2 is None else GuardedI(a.n)
    radii = None if rb2 is None else Radii(rb2)
    rc = lib.rg_radius_hits(a.ptr, a.ld, a.n, b.ptr, b.ld, b.n, a.F, None if radii is None else radii.ptr, ws.ptr, need,
                            None if count is None else count.t.data_ptr(), mind2.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert mind2.intact() and ws.intact() and (count is None or count.intact()), "rg_radius_hits wrote outside its outputs / workspace"
    return (None if count is None else count.t.cpu().numpy()), mind2.t.cpu().numpy()


_INT, _REF = {}, {}


def _ints(na, nb, F):
    if (na, nb, F) not in _INT:
        _INT[(na, nb, F)] = integer_case(na, nb, F, seed=1000 * F + 7 * na + nb)
    return _INT[(na, nb, F)]


def _ref(key, fn):
    """the restatement, computed once per case and shared by the builds"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _check_hits_exact(lib, a, b, key, what, ld_extra=0, shift=0):
    k = min(3, len(b) - 1)
    rb2 = _ref(key + ("rb2",), lambda: radii2_ref(b, k))
    wcount, wmin = _ref(key + ("hits",), lambda: hits_ref(a, b, rb2))
    da, db = Rows(a, a.shape[1] + ld_extra, shift), Rows(b, b.shape[1] + ld_extra, shift)
    count, mind2 = _hits(lib, da, db, rb2)
    assert count.dtype == np.int32 and np.array_equal(count, wcount), "%s: counts differ\n%r\n%r" % (what, count, wcount)
    assert _same_bits(mind2, wmin), "%s: minima differ\n%r\n%r" % (what, mind2, wmin)
    none, only = _hits(lib, da, db, None)
    assert none is None and _same_bits(only, wmin), what + " (minimum only)"


def _check_knn_exact(lib, a, ks, key, what, ld_extra=0, shift=0):
    da = Rows(a, a.shape[1] + ld_extra, shift)
    for k in ks:
        want = _ref(key + ("knn", k), lambda: radii2_ref(a, k))
        got = _knn(lib, da, k)
        assert _same_bits(got, want), "%s k=%d: radii differ\n%r\n%r" % (what, k, got, want)


def _ks(n):
    return sorted(set(k for k in (1, 3, 5, 16, n - 1) if 1 <= k <= min(16, n - 1)))


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", [33, 70])
def test_hits_every_row_count_pair(half, F):
    lib = _abi.load(half)
    for na in ROW_COUNTS:
        for nb in ROW_COUNTS:
            a, b = _ints(na, nb, F)
            _check_hits_exact(lib, a, b, ("hits", na, nb, F), "%s na=%d nb=%d F=%d" % (half, na, nb, F))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_hits_feature_counts_strides_and_alignment(half, F):
    lib = _abi.load(half)
    for na, nb in ((65, 63), (2, 130)):
        a, b = _ints(na, nb, F)
        for ld_extra, shift in STRIDES:
            _check_hits_exact(lib, a, b, ("hits", na, nb, F), "%s na=%d nb=%d F=%d ld=F+%d shift=%d" % (half, na, nb, F, ld_extra, shift),
                              ld_extra, shift)


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", [33, 70])
def test_knn_row_counts_and_every_k(half, F):
    """k in {1, 3, 5, 16} where the set has k + 1 rows, and k = n - 1 (n = 2, 6, 17: the radius is the farthest row)"""
    lib = _abi.load(half)
    for n in ROW_COUNTS + [6, 17]:
        a, _ = _ints(n, 1, F)
        assert n - 1 in _ks(n) or n > 17
        _check_knn_exact(lib, a, _ks(n), ("knn", n, F), "%s n=%d F=%d" % (half, n, F))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_knn_feature_counts_strides_and_alignment(half, F):
    lib = _abi.load(half)
    for n in (65, 130):
        a, _ = _ints(n, 1, F)
        for ld_extra, shift in STRIDES:
            _check_knn_exact(lib, a, (1, 5), ("knn", n, F), "%s n=%d F=%d ld=F+%d shift=%d" % (half, n, F, ld_extra, shift), ld_extra, shift)


@pytest.mark.parametrize("half", BUILDS)
def test_a_row_is_excluded_by_index_not_by_value(half):
    """rows (r, 0, 0): d2 = (r - s)^2, every first radius is 1 -- except where a duplicate sits at distance 0: rows 0 and 129
    (different tiles, the duplicate reaches row 0 through an off-diagonal tile) and rows 69 and 70 (one diagonal tile).  Excluding
    zero DISTANCES instead of the own INDEX would give those four rows a radius of 1 as well."""
    lib = _abi.load(half)
    a = np.zeros((130, 3), dtype=np.float32)
    a[:, 0] = np.arange(130)
    a[129] = a[0]
    a[70] = a[69]
    want = np.ones(130)
    want[[0, 129, 69, 70]] = 0.0
    assert np.array_equal(radii2_ref(a, 1), want)
    da = Rows(a, 3)
    assert np.array_equal(_knn(lib, da, 1), want)
    assert _same_bits(_knn(lib, da, 2), radii2_ref(a, 2)) and _same_bits(_knn(lib, da, 16), radii2_ref(a, 16))
    # a set against itself: every row hits itself (d2 = 0 <= any radius) and the minimum is 0
    count, mind2 = _hits(lib, da, da, want)
    wcount, _ = hits_ref(a, a, want)
    assert np.array_equal(count, wcount) and np.all(count >= 1) and np.array_equal(mind2, np.zeros(130))


# ------------------------------------------------------------------ general floats
_FLOATS = {}


def _floats():
    if not _FLOATS:
        rng = np.random.default_rng(77)
        a = rng.standard_normal((130, 70)).astype(np.float32)
        b = rng.standard_normal((70, 70)).astype(np.float32)
        g = GAMMA(70)
        rb2 = radii2_ref(b, 5)
        _FLOATS.update(a=a, b=b, rb2=rb2, ra2={k: radii2_ref(a, k) for k in (1, 5, 16)}, hits=hits_ref(a, b, rb2),
                       strict=hits_ref(a, b, rb2, 1.0 + 2.0 * g)[0], loose=hits_ref(a, b, rb2, 1.0 - 2.0 * g)[0])
    return _FLOATS


def _within(got, want, F, what):
    bound = 2.0 * GAMMA(F) * np.maximum(got, want)
    err = np.abs(got - want)
    print("%s: max |dev - ref| / (2 gamma max) = %.3g" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.isfinite(got).all() and np.all(err <= bound), what


@pytest.mark.parametrize("half", BUILDS)
def test_general_floats_within_the_rounding_bound(half):
    lib = _abi.load(half)
    ref = _floats()
    da, db = Rows(ref["a"], 75, 1), Rows(ref["b"], 70)
    for k in (1, 5, 16):
        got = _knn(lib, da, k)
        _within(got, ref["ra2"][k], 70, "%s radii k=%d" % (half, k))
        assert _same_bits(_knn(lib, da, k), got), "the same bits on every run"
    count, mind2 = _hits(lib, da, db, ref["rb2"])
    _within(mind2, ref["hits"][1], 70, half + " minima")
    print("%s counts: strict %d <= device %d <= loose %d (restatement %d)" % (
        half, ref["strict"].sum(), count.sum(), ref["loose"].sum(), ref["hits"][0].sum()))
    assert np.all(ref["strict"] <= count) and np.all(count <= ref["loose"])
    again, magain = _hits(lib, da, db, ref["rb2"])
    assert np.array_equal(again, count) and _same_bits(magain, mind2), "the same bits on every run"
    only = _hits(lib, da, db, None)[1]
    assert _same_bits(only, mind2), "the minimum-only form returns the minima of the full form"


# ------------------------------------------------------------------ symmetry, tiling, the minimum-only form
@pytest.mark.parametrize("half", BUILDS)
def test_distances_are_symmetric_and_independent_of_the_tiling(half):
    """The device's own d2 matrix, one column per minimum-only call against a 1-row b (d2(a_r, b_0) for every r): it is
    symmetric bit for bit with a zero diagonal, the transposed call (b_0 against all of a) returns the minimum of the same
    bits, and the radii selected from it on the host EQUAL rg_knn_radii2, whose tiles (64 x 64, upper triangle, read both ways)
    are other tiles than these 64 x 1 ones."""
    lib = _abi.load(half)
    a = _floats()["a"]
    n, F = a.shape
    da = Rows(a, F + 5, 3)
    D = np.empty((n, n))
    need = lib.rg_pairdist_ws_bytes(n, 1, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty(n, n, dtype=torch.float64, device=DEV)
    for s in range(n):
        rc = lib.rg_radius_hits(da.ptr, da.ld, n, da.ptr + 4 * s * da.ld, da.ld, 1, F, None, ws.data_ptr(), need, None,
                                out[s].data_ptr(), None)
        assert rc == 0, lib.rg_last_error()
    torch.cuda.synchronize()
    D = out.cpu().numpy().T                                  # D[r][s] = d2(a_r, a_s)
    assert np.isfinite(D).all() and np.all(D >= 0.0) and np.all(np.diagonal(D) == 0.0)
    assert _same_bits(D, D.T), "d2(a, b) and d2(b, a) must hold the same bits"
    for s in (0, 63, 64, 129):
        one = Rows(a[s:s + 1], F)
        _, m = _hits(lib, one, da, None)
        assert m.shape == (1,) and m[0] == 0.0
        others = Rows(np.delete(a, s, axis=0), F)
        _, m = _hits(lib, one, others, None)
        assert m[0] == np.delete(D[:, s], s).min(), "the transposed pairs' minimum differs from the minimum of the same d2 values"
    for k in (1, 5, 16):
        want = np.array([np.sort(np.delete(D[i], i))[k - 1] for i in range(n)])
        assert _same_bits(_knn(lib, da, k), want), "k=%d: rg_knn_radii2 differs from a selection over rg_radius_hits' own d2" % k
    # ... and the counts are those of the same matrix
    rb2 = _floats()["ra2"][5]
    count, mind2 = _hits(lib, da, da, rb2)
    assert np.array_equal(count, (D <= rb2[None, :]).sum(axis=1)) and np.array_equal(mind2, np.zeros(n))


@pytest.mark.parametrize("half", BUILDS)
def test_a_nan_row_never_hits_and_leaves_the_finite_rows_alone(half):
    lib = _abi.load(half)
    ref = _floats()
    a, b = ref["a"].copy(), ref["b"].copy()
    a[66, 3] = np.nan                                         # one NaN feature is enough
    b[5, :] = np.nan
    keep_a, keep_b = np.delete(np.arange(130), 66), np.delete(np.arange(70), 5)
    da, db = Rows(a, 70), Rows(b, 70)
    for k in (1, 5):
        got = _knn(lib, da, k)
        assert got[66] == np.inf, "the NaN row's own radius"
        assert _same_bits(got[keep_a], _knn(lib, Rows(a[keep_a], 70), k)), "a NaN row moved the radii of finite rows"
    rb2 = np.full(70, np.inf)                                 # even an infinite radius is not hit by a NaN distance
    count, mind2 = _hits(lib, da, db, rb2)
    assert count[66] == 0 and mind2[66] == np.inf
    assert np.all(count[keep_a] == 69), "every finite pair hits an infinite radius, the NaN row of b is hit by nobody"
    clean_count, clean_min = _hits(lib, Rows(a[keep_a], 70), Rows(b[keep_b], 70), ref["rb2"][keep_b])
    rb2 = ref["rb2"].copy()
    count, mind2 = _hits(lib, da, db, rb2)
    assert np.array_equal(count[keep_a], clean_count) and _same_bits(mind2[keep_a], clean_min)
    # a set of NaN rows only: radii and minima are +inf, counts 0
    allnan = Rows(np.full((3, 70), np.nan, dtype=np.float32), 70)
    assert np.all(_knn(lib, allnan, 2) == np.inf)
    count, mind2 = _hits(lib, da, allnan, np.full(3, np.inf))
    assert np.all(count == 0) and np.all(mind2 == np.inf)


# ------------------------------------------------------------------ contracts
@pytest.mark.parametrize("half", BUILDS)
def test_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    F, na, nb, k = 17, 70, 5, 3
    a, b = _ints(na, nb, F)
    da, db = Rows(a, F + 5), Rows(b, F + 2)
    need_k, need_h = lib.rg_pairdist_ws_bytes(na, na, k), lib.rg_pairdist_ws_bytes(na, nb, 0)
    assert need_k == 2 * na * k * 8 and need_h == 1 * na * 12
    assert lib.rg_pairdist_ws_bytes(64, 64, 16) == 64 * 16 * 8 and lib.rg_pairdist_ws_bytes(65, 130, 0) == 3 * 65 * 12
    assert lib.rg_pairdist_ws_bytes(0, 5, 0) == 0 and lib.rg_pairdist_ws_bytes(-1, 5, 3) == 0 and lib.rg_pairdist_ws_bytes(5, 5, 17) == 0
    ws, r2, count, mind2 = GuardedWS(max(need_k, need_h)), GuardedD((na,)), GuardedI(na), GuardedD((na,))
    rad = Radii(np.ones(nb))
    pr, pc, pm, big, huge = r2.t.data_ptr(), count.t.data_ptr(), mind2.t.data_ptr(), 2 ** 31 - 1, ctypes.c_size_t(-1).value

    def untouched(what):
        torch.cuda.synchronize()
        assert ws.untouched() and r2.untouched() and count.untouched() and mind2.untouched(), what

    #               a       lda    n   F   k   ws      bytes   r2  code
    bad = {"F = 0": (da.ptr, da.ld, na, 0, k, ws.ptr, need_k, pr, EINVAL),
           "F < 0": (da.ptr, da.ld, na, -3, k, ws.ptr, need_k, pr, EINVAL),
           "n < 0": (da.ptr, da.ld, -1, F, k, ws.ptr, need_k, pr, EINVAL),
           "lda < F": (da.ptr, F - 1, na, F, k, ws.ptr, need_k, pr, EINVAL),
           "k = 0": (da.ptr, da.ld, na, F, 0, ws.ptr, need_k, pr, EINVAL),
           "k = 17": (da.ptr, da.ld, na, F, 17, ws.ptr, huge, pr, EINVAL),
           "k < 0": (da.ptr, da.ld, na, F, -1, ws.ptr, need_k, pr, EINVAL),
           "n = k": (da.ptr, da.ld, k, F, k, ws.ptr, need_k, pr, EINVAL),
           "n = 0": (da.ptr, da.ld, 0, F, 1, ws.ptr, need_k, pr, EINVAL),
           "a = NULL": (None, da.ld, na, F, k, ws.ptr, need_k, pr, EINVAL),
           "ws = NULL": (da.ptr, da.ld, na, F, k, None, need_k, pr, EINVAL),
           "r2 = NULL": (da.ptr, da.ld, na, F, k, ws.ptr, need_k, None, EINVAL),
           "ws one byte short": (da.ptr, da.ld, na, F, k, ws.ptr, need_k - 1, pr, EWORKSPACE),
           "ws of 0 bytes": (da.ptr, da.ld, na, F, k, ws.ptr, 0, pr, EWORKSPACE),
           "too many tiles": (da.ptr, 1, big, 1, 1, ws.ptr, huge, pr, EUNSUPPORTED)}
    for what, (pa, lda, n, f, kk, w, wb, r, code) in bad.items():
        rc = lib.rg_knn_radii2(pa, lda, n, f, kk, w, wb, r, None)
        assert rc == code, "rg_knn_radii2, %s: returned %d" % (what, rc)
        assert b"knn_radii2" in lib.rg_last_error(), what
        untouched("rg_knn_radii2, " + what)
    #               a       lda    na  b       ldb    nb  F  rb2      ws      bytes   count mind2 code
    bad = {"F = 0": (da.ptr, da.ld, na, db.ptr, db.ld, nb, 0, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "na < 0": (da.ptr, da.ld, -1, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "nb < 0": (da.ptr, da.ld, na, db.ptr, db.ld, -1, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "lda < F": (da.ptr, F - 1, na, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "ldb < F": (da.ptr, da.ld, na, db.ptr, F - 1, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "a = NULL": (None, da.ld, na, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "b = NULL": (da.ptr, da.ld, na, None, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, EINVAL),
           "ws = NULL": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, rad.ptr, None, need_h, pc, pm, EINVAL),
           "mind2 = NULL": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, None, EINVAL),
           "mind2 = NULL, minimum only": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, None, ws.ptr, need_h, None, None, EINVAL),
           "count without rb2": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, None, ws.ptr, need_h, pc, pm, EINVAL),
           "rb2 without count": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, None, pm, EINVAL),
           "count without rb2, no rows": (da.ptr, da.ld, 0, db.ptr, db.ld, nb, F, None, ws.ptr, need_h, pc, pm, EINVAL),
           "ws one byte short": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h - 1, pc, pm, EWORKSPACE),
           "ws one byte short, minimum only": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, None, ws.ptr, need_h - 1, None, pm, EWORKSPACE),
           "too many tiles": (da.ptr, 1, big, db.ptr, 1, big, 1, rad.ptr, ws.ptr, huge, pc, pm, EUNSUPPORTED)}
    for what, args in bad.items():
        rc = lib.rg_radius_hits(*args[:-1], None)
        assert rc == args[-1], "rg_radius_hits, %s: returned %d" % (what, rc)
        assert b"radius_hits" in lib.rg_last_error(), what
        untouched("rg_radius_hits, " + what)
    # an empty operand: RG_OK, nothing written, no buffers needed
    assert lib.rg_radius_hits(da.ptr, da.ld, 0, db.ptr, db.ld, nb, F, rad.ptr, ws.ptr, need_h, pc, pm, None) == 0
    assert lib.rg_radius_hits(da.ptr, da.ld, na, db.ptr, db.ld, 0, F, rad.ptr, ws.ptr, need_h, pc, pm, None) == 0
    assert lib.rg_radius_hits(None, F, 0, None, F, 0, F, None, None, 0, None, None, None) == 0
    untouched("empty operands")
    # the minimum-only form has no count to touch: a real launch leaves a neighbouring count buffer alone
    assert lib.rg_radius_hits(da.ptr, da.ld, na, db.ptr, db.ld, nb, F, None, ws.ptr, need_h, None, pm, None) == 0
    torch.cuda.synchronize()
    assert count.untouched() and r2.untouched() and mind2.intact() and ws.intact() and bool((mind2.t != DSENT).all())
    assert _same_bits(mind2.t.cpu().numpy(), hits_ref(a, b)[1])


@pytest.mark.parametrize("half", BUILDS)
def test_graph_replay_equals_eager(half):
    """both entry points captured on one stream into one graph (no host synchronisation, no allocation inside), replayed twice"""
    lib = _abi.load(half)
    ref = _floats()
    da, db = Rows(ref["a"], 75, 1), Rows(ref["b"], 70)
    want_r = _knn(lib, db, 5)
    want_c, want_m = _hits(lib, da, db, want_r)
    need = max(lib.rg_pairdist_ws_bytes(70, 70, 5), lib.rg_pairdist_ws_bytes(130, 70, 0))
    ws, r2, count, mind2 = GuardedWS(need), GuardedD((70,)), GuardedI(130), GuardedD((130,))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.rg_knn_radii2(db.ptr, db.ld, 70, 70, 5, ws.ptr, need, r2.t.data_ptr(), st) == 0, lib.rg_last_error()
        assert lib.rg_radius_hits(da.ptr, da.ld, 130, db.ptr, db.ld, 70, 70, r2.t.data_ptr(), ws.ptr, need, count.t.data_ptr(),
                                  mind2.t.data_ptr(), st) == 0, lib.rg_last_error()
    for _ in range(2):
        r2.t.fill_(DSENT); mind2.t.fill_(DSENT); count.t.fill_(SBITS)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(r2.t.cpu().numpy(), want_r) and _same_bits(mind2.t.cpu().numpy(), want_m)
        assert np.array_equal(count.t.cpu().numpy(), want_c)
        assert r2.intact() and mind2.intact() and count.intact() and ws.intact()
