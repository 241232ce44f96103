"""rg_polykernel_tile_sums (include/rnagan_hip.h, rna_gan_amd/csrc/rg_fidstat.hip) op by op through ctypes, on both builds of
the library, against the numpy restatement of tests/kid_refs.py (pinned without a GPU by tests/test_kid_refs_cpu.py).

Operands live inside NaN-filled allocations (a column past F that is read shows as a non-finite sum; such reads stay inside the
allocation, so nothing can fault); sums and diag live inside allocations pre-filled with one finite pattern, THEMSELVES
included: the kernel writes, it does not accumulate, and what it must leave alone keeps the pattern.

Exact cases: integer features in [-3, 3].  Every value and every tile sum of the contract is then exactly representable (proved
with fractions.Fraction for the two cases of the issue by the CPU test; for gamma = 1 and F <= 256 the values are integers below
2305^3 and a tile's sum stays below 2^53), so any summation order gives the same bits and the result must EQUAL the restatement.
Shapes: row counts around the 64-row tile (1, 63, 64, 65) and over three tiles with a ragged last one (130), in every
combination; feature counts around the kernel's 32-feature staging pass (1, 31, 32, 33), over three passes with a ragged last
one (70) and over eight (256); lda = F and F + 5 (rows that start at odd addresses) and a base pointer 4 bytes off alignment.

General floats: the terms are restated bit for bit, only the order of a tile's <= 4096 additions is the kernel's own, so
|got - fsum| <= 4096 * 2^-53 * sum |v| per tile (the first-order bound (n - 1) u sum |v| for n terms in any order, n <= 4096;
fsum's own rounding, u |sum|, is inside the slack between n - 1 and n); diag has at most 64 terms: 64 * 2^-53 * sum |v|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from guarded import DEV, Guarded
from kid_refs import TILE, U, integer_case, tile_abs_sums_ref, tile_sums_ref
from vae_fid_refs import SENTINEL

BUILDS = ["bf16", "f16"]
DSENT = float(SENTINEL)
ROW_COUNTS = [1, 63, 64, 65, 130]
F_SIZES = [1, 31, 32, 33, 70, 256]


def _tiles(n):
    return (n + TILE - 1) // TILE


class GuardedD:
    """`shape` doubles in the middle of an fp64 allocation filled with DSENT, the doubles themselves included"""

    def __init__(self, shape, pad=512):
        n = int(np.prod(shape))
        self.flat = torch.full((pad + n + pad,), DSENT, dtype=torch.float64, device=DEV)
        self.t = self.flat[pad:pad + n].view(shape)
        self.pad, self.n = pad, n

    def intact(self):
        return bool((self.flat[:self.pad] == DSENT).all()) and bool((self.flat[self.pad + self.n:] == DSENT).all())

    def untouched(self):
        return bool((self.flat == DSENT).all())


class Rows:
    """x (n, F) fp32 inside a NaN-filled allocation with row stride ld, the first row `shift` floats past a 256-byte boundary:
    columns past F, rows past n and everything around are NaN"""

    def __init__(self, x, ld, shift=0):
        n, F = x.shape
        self.g = Guarded(torch.full((shift + (n + 40) * ld,), float("nan"), dtype=torch.float32), float("nan"), before=128, after=4096)
        self.rows = self.g.t[shift:].view(n + 40, ld)
        self.rows[:n, :F] = torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV)
        self.ptr, self.ld, self.n, self.F = self.rows.data_ptr(), ld, n, F
        assert self.ptr % 256 == (4 * shift) % 256


def _call(lib, a, b, gamma, coef0, degree):
    """one launch -> (sums, diag or None) as numpy fp64; checks the return code and that nothing outside the outputs was written"""
    ta, tb = _tiles(a.n), _tiles(a.n if b is None else b.n)
    sums = GuardedD((ta, tb))
    diag = GuardedD((ta,)) if b is None else None
    rc = lib.rg_polykernel_tile_sums(a.ptr, a.ld, a.n, None if b is None else b.ptr, 0 if b is None else b.ld,
                                     0 if b is None else b.n, a.F, gamma, coef0, degree, sums.t.data_ptr(),
                                     None if diag is None else diag.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert sums.intact() and (diag is None or diag.intact()), "rg_polykernel_tile_sums wrote outside sums / diag"
    return sums.t.cpu().numpy(), (None if diag is None else diag.t.cpu().numpy())


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


_INT, _REF = {}, {}


def _ints(na, nb, F):
    if (na, nb, F) not in _INT:
        _INT[(na, nb, F)] = integer_case(na, nb, F, seed=1000 * F + 7 * na + nb)
    return _INT[(na, nb, F)]


def _ref(key, a, b, gamma, coef0, degree):
    """the restatement, computed once per case and shared by the builds"""
    if key not in _REF:
        _REF[key] = tile_sums_ref(a, b, gamma, coef0, degree)
    return _REF[key]


def _check_exact(lib, a, b, gamma, degree, key, what, ld_extra=0, shift=0):
    """two-operand (a, b) and symmetric (a) calls against the restatement, bit for bit"""
    da, db = Rows(a, a.shape[1] + ld_extra, shift), Rows(b, b.shape[1] + ld_extra, shift)
    want, _ = _ref(key + ("ab", degree), a, b, gamma, 1.0, degree)
    got, none = _call(lib, da, db, gamma, 1.0, degree)
    assert none is None and np.isfinite(got).all(), what + ": a column outside the operands was read"
    assert _same_bits(got, want), "%s: tile sums differ from the restatement\n%r\n%r" % (what, got, want)
    want, wdiag = _ref(key + ("aa", degree), a, None, gamma, 1.0, degree)
    got, gdiag = _call(lib, da, None, gamma, 1.0, degree)
    assert np.isfinite(got).all() and np.isfinite(gdiag).all(), what
    assert _same_bits(got, want), "%s (symmetric): tile sums differ from the restatement\n%r\n%r" % (what, got, want)
    assert _same_bits(gdiag, wdiag), "%s (symmetric): diag differs from the restatement" % what
    assert _same_bits(got, got.T), what


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F,gamma", [(64, 1.0 / 64), (70, 1.0)])
def test_integer_cases_bit_equal(half, F, gamma):
    """the two cases whose exactness tests/test_kid_refs_cpu.py proves: na = 130, nb = 70, degrees 1, 2 and 3"""
    lib = _abi.load(half)
    a, b = integer_case(130, 70, F, seed=F)
    for degree in (1, 2, 3):
        _check_exact(lib, a, b, gamma, degree, ("issue", F), "%s F=%d degree=%d" % (half, F, degree))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("na", ROW_COUNTS)
def test_row_counts(half, na):
    lib = _abi.load(half)
    for nb in ROW_COUNTS:
        a, b = _ints(na, nb, 70)
        _check_exact(lib, a, b, 1.0, 3, ("rows", na, nb), "%s na=%d nb=%d" % (half, na, nb))


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_feature_counts_strides_and_alignment(half, F):
    lib = _abi.load(half)
    a, b = _ints(65, 63, F)
    for degree in (1, 2, 3):
        for ld_extra, shift in ((0, 0), (5, 0), (0, 1), (5, 3)):
            _check_exact(lib, a, b, 1.0, degree, ("F", F), "%s F=%d degree=%d ld=F+%d shift=%d" % (half, F, degree, ld_extra, shift),
                         ld_extra, shift)


@pytest.mark.parametrize("half", BUILDS)
def test_position_map(half):
    """one-hot rows: k(a_r, b_s) = 1 + [c(r) == c(s)] w_r w_s at degree 1, so a tile sum written to a transposed or shifted place,
    or a masked row that leaked in, shows; a (130, 70) problem has a 3 x 2 tile matrix that is asymmetric in shape as well"""
    lib = _abi.load(half)
    F = 33
    a = np.zeros((130, F), dtype=np.float32)
    b = np.zeros((70, F), dtype=np.float32)
    for r in range(130):
        a[r, (7 * r) % F] = r + 1
    for s in range(70):
        b[s, (5 * s) % F] = -(s + 2)
    _check_exact(lib, a, b, 1.0, 1, ("onehot",), half + " one-hot rows")
    # coef0 = 0 at degree 1 is the plain Gram sum: rows past the end contribute nothing, k(0, y) = 0 then -- and with coef0 = 1
    # each tile's sum exceeds it by exactly the number of (unmasked) pairs
    da, db = Rows(a, F), Rows(b, F)
    plain, _ = _call(lib, da, db, 1.0, 0.0, 1)
    ones, _ = _call(lib, da, db, 1.0, 1.0, 1)
    pairs = np.outer([64, 64, 2], [64, 6]).astype(np.float64)
    assert np.array_equal(ones - plain, pairs)


# ------------------------------------------------------------------ general floats
_FLOATS = {}


def _floats():
    if not _FLOATS:
        rng = np.random.default_rng(77)
        a = rng.standard_normal((130, 70)).astype(np.float32)
        b = rng.standard_normal((70, 70)).astype(np.float32)
        _FLOATS["ab"] = (a, b)
        for degree in (1, 2, 3):
            for form, rhs in (("ab", b), ("aa", None)):
                _FLOATS[(form, degree)] = (tile_sums_ref(a, rhs, 1.0 / 70, 1.0, degree), tile_abs_sums_ref(a, rhs, 1.0 / 70, 1.0, degree))
    return _FLOATS


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_general_floats_within_the_summation_bound(half, degree):
    lib = _abi.load(half)
    ref = _floats()
    a, b = ref["ab"]
    da, db = Rows(a, 75, 1), Rows(b, 70)
    (want, _), (scale, _) = ref[("ab", degree)]
    got, _ = _call(lib, da, db, 1.0 / 70, 1.0, degree)
    err = np.abs(got - want)
    print("%s degree %d: two operands, max |got - fsum| / (4096 u sum|v|) = %.3g" % (half, degree, float((err / (4096 * U * scale)).max())))
    assert np.isfinite(got).all() and np.all(err <= 4096 * U * scale)
    # symmetric form
    (want, wdiag), (scale, sdiag) = ref[("aa", degree)]
    sym, diag = _call(lib, da, None, 1.0 / 70, 1.0, degree)
    err, derr = np.abs(sym - want), np.abs(diag - wdiag)
    print("%s degree %d: symmetric, max ratio %.3g, diag ratio %.3g" % (
        half, degree, float((err / (4096 * U * scale)).max()), float((derr / (64 * U * sdiag)).max())))
    assert np.all(err <= 4096 * U * scale) and np.all(derr <= 64 * U * sdiag)
    assert _same_bits(sym, sym.T), "sums[i][j] and sums[j][i] must hold the same bits"
    # ... and equals the two-operand call on (a, a) bit for bit (the tile's summation order is transposition invariant)
    two, _ = _call(lib, da, Rows(a, 70), 1.0 / 70, 1.0, degree)
    assert _same_bits(two, sym), "the symmetric form must return the bits of the two-operand call on (a, a)"
    # the same bits on every run
    again, dagain = _call(lib, da, None, 1.0 / 70, 1.0, degree)
    assert _same_bits(again, sym) and _same_bits(dagain, diag)
    again, _ = _call(lib, da, db, 1.0 / 70, 1.0, degree)
    assert _same_bits(again, got)


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("half", BUILDS)
def test_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    F, na, nb = 17, 70, 5
    a, b = _ints(na, nb, F)
    da, db = Rows(a, F + 5), Rows(b, F + 2)
    sums, diag = GuardedD((2, 2)), GuardedD((2,))
    ps, pd = sums.t.data_ptr(), diag.t.data_ptr()
    big = 2 ** 31 - 1
    #        a       lda     na  b       ldb     nb  F  degree sums diag  code
    bad = {"F = 0": (da.ptr, da.ld, na, db.ptr, db.ld, nb, 0, 3, ps, None, -1),
           "F < 0": (da.ptr, da.ld, na, db.ptr, db.ld, nb, -4, 3, ps, None, -1),
           "na < 0": (da.ptr, da.ld, -1, db.ptr, db.ld, nb, F, 3, ps, None, -1),
           "nb < 0": (da.ptr, da.ld, na, db.ptr, db.ld, -1, F, 3, ps, None, -1),
           "lda < F": (da.ptr, F - 1, na, db.ptr, db.ld, nb, F, 3, ps, None, -1),
           "ldb < F": (da.ptr, da.ld, na, db.ptr, F - 1, nb, F, 3, ps, None, -1),
           "lda < F, symmetric": (da.ptr, F - 1, na, None, 0, 0, F, 3, ps, pd, -1),
           "degree 0": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, 0, ps, None, -1),
           "degree 4": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, 4, ps, None, -1),
           "degree -1, symmetric": (da.ptr, da.ld, na, None, 0, 0, F, -1, ps, pd, -1),
           "a = NULL": (None, da.ld, na, db.ptr, db.ld, nb, F, 3, ps, None, -1),
           "sums = NULL": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, 3, None, None, -1),
           "sums = NULL, symmetric": (da.ptr, da.ld, na, None, 0, 0, F, 3, None, pd, -1),
           "diag = NULL, symmetric": (da.ptr, da.ld, na, None, 0, 0, F, 3, ps, None, -1),
           "diag with two operands": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, 3, ps, pd, -1),
           "too many tiles": (da.ptr, 1, big, db.ptr, 1, big, 1, 3, ps, None, -2),
           "too many tiles, symmetric": (da.ptr, 1, big, None, 0, 0, 1, 3, ps, pd, -2)}
    for what, (pa, lda, n1, pb, ldb, n2, f, degree, s, d, code) in bad.items():
        rc = lib.rg_polykernel_tile_sums(pa, lda, n1, pb, ldb, n2, f, 1.0 / F, 1.0, degree, s, d, None)
        torch.cuda.synchronize()
        assert rc == code, "%s: returned %d" % (what, rc)
        assert b"polykernel_tile_sums" in lib.rg_last_error(), what
        assert sums.untouched() and diag.untouched(), what
    # an empty operand: RG_OK, nothing written, no buffers needed
    for n1, pb, n2, d in ((0, db.ptr, nb, None), (na, db.ptr, 0, None), (0, None, 0, pd)):
        assert lib.rg_polykernel_tile_sums(da.ptr, da.ld, n1, pb, db.ld, n2, F, 1.0 / F, 1.0, 3, ps, d, None) == 0
    assert lib.rg_polykernel_tile_sums(None, F, 0, None, 0, 0, F, 1.0, 1.0, 3, None, pd, None) == 0
    torch.cuda.synchronize()
    assert sums.untouched() and diag.untouched()
    # the two-operand form has no diag to touch: a neighbouring diag-sized buffer keeps its pattern through a real launch
    two = GuardedD((2, 1))
    assert lib.rg_polykernel_tile_sums(da.ptr, da.ld, na, db.ptr, db.ld, nb, F, 1.0 / F, 1.0, 3, two.t.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert two.intact() and diag.untouched() and bool((two.t != DSENT).all())
