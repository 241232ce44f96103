"""rg_group_sums_update and rg_match_ranks (include/rnagan_hip.h, rna_gan_amd/csrc/rg_groupstat.hip) op by op through ctypes, on
both builds of the library, against the numpy restatements of tests/repr_refs.py (pinned without a GPU by
tests/test_repr_refs_cpu.py).

Operands live inside NaN-filled allocations (a row or column read past the operand shows as a NaN sum or distance; such reads stay
inside the allocation, so nothing can fault); the group ids are surrounded by id 0 and the targets by a huge index (an id or a
target read past the end would be counted, or clamped to the last row).  Outputs live inside allocations pre-filled with one
pattern: what is outside them must keep it.

rg_group_sums_update: the contract is ONE chain of fp64 additions per entry in row order, so the sums must EQUAL the sequential
restatement bit for bit on general floats (80 binades, both signs: the additions round, so their order shows), whatever the
split of the rows over calls.  Row counts around the 64-id ballot (1, 63, 64, 65), over three of them (130) and over three staging passes of 1024 ids with a ragged last one (2100);
feature counts 1, 31, 32, 33, 70 and past one 256-column workgroup (300); G = 1, 2, 7, 65.

rg_match_ranks: integer-valued rows in [-3, 3] make every d2 an exact integer, so ranks and d* must EQUAL the restatement, ties
included (repr_refs.integer_rows plants duplicates of the target row on both sides of the target index).  na, nb around the 64-row
tile and over three tiles; nb <= 64 takes the path that writes rank directly, nb > 64 the one that shares the tiles of b out and
adds with integer atomics; 65 x 8262 makes two of the 128 parts walk a second tile.  General floats: device and restatement are
each within GAMMA(F) of the exact d2 (prdc_refs.GAMMA), so |d*_dev - d*_ref| <= 2 GAMMA max and the device rank lies between the
restatement's ranks at d* (1 - 2 GAMMA) and d* (1 + 2 GAMMA).

The float and the double distance paths: rg_radius_hits on fp32 rows and rg_match_ranks on the same rows widened to fp64 are the
same sequence of fp64 operations on the same values (rna_gan_amd/csrc/rg_pairtile.h; zero padding is fma(0, 0, acc) = acc), so
their d2 must hold the same bits on general floats -- no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from guarded import DEV, SBITS
from prdc_refs import GAMMA
from repr_refs import dist2_f64, group_sums_ref, integer_rows, match_ranks_ref, ranks_from_d2, wide_floats
from test_kid_ops_gpu import DSENT, GuardedD, Rows, _same_bits
from test_prdc_ops_gpu import GuardedI

BUILDS = ["bf16", "f16"]
ROW_COUNTS = [1, 63, 64, 65, 130]
F_SIZES = [1, 31, 32, 33, 70]
GROUPS = [1, 2, 7, 65]
MATCH_ROWS = [1, 2, 63, 64, 65, 130]
STRIDES = ((0, 0), (5, 0), (0, 1), (5, 3))                  # (ld - F, elements the base pointer is off a 256-byte boundary)
PATTERNS = ("interleaved", "sorted", "one", "gaps", "planted")
EINVAL, EUNSUPPORTED = -1, -2
LSENT = 0x5e59e2d35e59e2d3
BAD_TARGET = 1 << 30


class GuardedL:
    """n int64 in the middle of an allocation filled with LSENT, the n themselves included"""

    def __init__(self, n, pad=512):
        self.flat = torch.full((pad + n + pad,), LSENT, dtype=torch.int64, device=DEV)
        self.t, self.pad, self.n = self.flat[pad:pad + n], pad, n

    def intact(self):
        return bool((self.flat[:self.pad] == LSENT).all()) and bool((self.flat[self.pad + self.n:] == LSENT).all())

    def untouched(self):
        return bool((self.flat == LSENT).all())


class Ints:
    """an int32 operand inside an allocation filled with `fill`"""

    def __init__(self, v, fill, pad=256):
        v = np.asarray(v, dtype=np.int32)
        self.flat = torch.full((pad + len(v) + pad,), fill, dtype=torch.int32, device=DEV)
        self.flat[pad:pad + len(v)] = torch.from_numpy(v).to(DEV)
        self.ptr = self.flat.data_ptr() + 4 * pad


class RowsD:
    """x (n, F) fp64 inside a NaN-filled allocation with row stride ld, the first row `shift` doubles past a 256-byte boundary"""

    def __init__(self, x, ld, shift=0):
        n, F = x.shape
        self.flat = torch.full((32 + shift + (n + 40) * ld + 512,), float("nan"), dtype=torch.float64, device=DEV)
        self.rows = self.flat[32 + shift:32 + shift + (n + 40) * ld].view(n + 40, ld)
        self.rows[:n, :F] = torch.from_numpy(np.array(x, dtype=np.float64)).to(DEV)
        self.ptr, self.ld, self.n, self.F = self.rows.data_ptr(), ld, n, F
        assert self.ptr % 256 == (8 * shift) % 256


def _ids(pattern, n, G, seed):
    """(ids, x override rows): the id patterns of the module docstring; "planted" marks rows with ids -1 and G, which hold NaN"""
    r = np.arange(n)
    rng = np.random.default_rng(seed)
    if pattern == "interleaved":
        return (r % G).astype(np.int32)
    if pattern == "sorted":
        return np.sort(rng.integers(0, G, size=n)).astype(np.int32)
    if pattern == "one":
        return np.full(n, G - 1, dtype=np.int32)
    if pattern == "gaps":                                    # only every third group has rows
        return ((r % ((G + 2) // 3)) * 3 % G).astype(np.int32)
    ids = rng.integers(0, G, size=n).astype(np.int32)
    ids[::5] = -1
    ids[3::7] = G
    return ids


_CASES = {}


def _case(n, F, G, pattern):
    """(x, ids, want sums, want counts) from zero, computed once and shared by the builds"""
    key = (n, F, G, pattern)
    if key not in _CASES:
        x = wide_floats(n, F, seed=1000 * n + 10 * F + G)
        ids = _ids(pattern, n, G, seed=n + F + G)
        if pattern == "planted":
            x[(ids < 0) | (ids >= G)] = np.nan
        _CASES[key] = (x, ids) + group_sums_ref(x, ids, G)
    return _CASES[key]


def _sums(lib, x, ids, G, ld_extra=0, shift=0, start=None, cuts=()):
    """rg_group_sums_update over the rows of x, in one call or cut at `cuts` -> (sums, counts) as numpy; return codes and the
    guards of both outputs checked.  start: (sums, counts) the outputs hold before the first call (default zeros)."""
    n, F = x.shape
    dx, dg = Rows(x, F + ld_extra, shift), Ints(ids, 0)
    sums, counts = GuardedD((G, F)), GuardedL(G)
    sums.t.copy_(torch.from_numpy(np.zeros((G, F)) if start is None else start[0]).to(DEV))
    counts.t.copy_(torch.from_numpy(np.zeros(G, dtype=np.int64) if start is None else start[1]).to(DEV))
    edges = [0] + list(cuts) + [n]
    for r0, r1 in zip(edges[:-1], edges[1:]):
        rc = lib.rg_group_sums_update(dx.ptr + 4 * r0 * dx.ld, dx.ld, r1 - r0, F, dg.ptr + 4 * r0, G, sums.t.data_ptr(),
                                      counts.t.data_ptr(), None)
        assert rc == 0, lib.rg_last_error()
    torch.cuda.synchronize()
    assert sums.intact() and counts.intact(), "rg_group_sums_update wrote outside sums / counts"
    return sums.t.cpu().numpy(), counts.t.cpu().numpy()


# ------------------------------------------------------------------ rg_group_sums_update
@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_group_sums_equal_the_sequential_chain(half, F):
    lib = _abi.load(half)
    for n in ROW_COUNTS:
        for G in GROUPS:
            for pattern in PATTERNS:
                x, ids, wsums, wcounts = _case(n, F, G, pattern)
                sums, counts = _sums(lib, x, ids, G)
                what = "%s n=%d F=%d G=%d %s" % (half, n, F, G, pattern)
                assert counts.dtype == np.int64 and np.array_equal(counts, wcounts), "%s: counts\n%r\n%r" % (what, counts, wcounts)
                assert np.isfinite(sums).all(), what + ": a row of another group, an ignored row or a column past F was summed"
                assert _same_bits(sums, wsums), what + ": sums differ from the sequential chain"
                if pattern == "planted":
                    assert counts.sum() == int(((ids >= 0) & (ids < G)).sum()) < n


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES + [300])
def test_group_sums_strides_and_alignment(half, F):
    lib = _abi.load(half)
    for n, G in ((130, 7), (65, 2)):
        x, ids, wsums, wcounts = _case(n, F, G, "planted")
        for ld_extra, shift in STRIDES:
            sums, counts = _sums(lib, x, ids, G, ld_extra, shift)
            assert np.array_equal(counts, wcounts) and _same_bits(sums, wsums), "%s n=%d F=%d ld=F+%d shift=%d" % (half, n, F, ld_extra, shift)


@pytest.mark.parametrize("half", BUILDS)
def test_group_sums_continue_across_calls(half):
    """a split of the rows at every boundary gives the bits of one call; non-zero starting sums are continued, not overwritten;
    2100 rows: three staging passes of group ids"""
    lib = _abi.load(half)
    for n, F, G in ((130, 33, 7), (65, 70, 2), (2100, 5, 7)):
        x, ids, wsums, wcounts = _case(n, F, G, "planted")
        one = _sums(lib, x, ids, G)
        assert _same_bits(one[0], wsums) and np.array_equal(one[1], wcounts)
        for cut in (1, 63, 64):
            if cut < n:
                got = _sums(lib, x, ids, G, cuts=(cut,))
                assert _same_bits(got[0], wsums) and np.array_equal(got[1], wcounts), "%s n=%d cut at %d" % (half, n, cut)
        got = _sums(lib, x, ids, G, ld_extra=5, shift=1, cuts=(1, 63, 64))
        assert _same_bits(got[0], wsums) and np.array_equal(got[1], wcounts)
        start = (wide_floats(G, F, seed=5).astype(np.float64) * 1.0000001, np.arange(G, dtype=np.int64) * (1 << 33) + 3)
        want = group_sums_ref(x, ids, G, *start)
        got = _sums(lib, x, ids, G, start=start, cuts=(64,))
        assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), "starting values must be continued"
        assert not _same_bits(want[0], wsums)


@pytest.mark.parametrize("half", BUILDS)
def test_group_sums_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    n, F, G = 70, 17, 5
    x, ids, _, _ = _case(n, F, G, "interleaved")
    dx, dg = Rows(x, F + 3), Ints(ids, 0)
    sums, counts = GuardedD((G, F)), GuardedL(G)
    ps, pc, big = sums.t.data_ptr(), counts.t.data_ptr(), 2 ** 31 - 1
    #             x       ldx    n  F  group   G  sums counts code
    bad = {"F = 0": (dx.ptr, dx.ld, n, 0, dg.ptr, G, ps, pc, EINVAL),
           "F < 0": (dx.ptr, dx.ld, n, -2, dg.ptr, G, ps, pc, EINVAL),
           "G = 0": (dx.ptr, dx.ld, n, F, dg.ptr, 0, ps, pc, EINVAL),
           "G < 0": (dx.ptr, dx.ld, n, F, dg.ptr, -1, ps, pc, EINVAL),
           "n < 0": (dx.ptr, dx.ld, -1, F, dg.ptr, G, ps, pc, EINVAL),
           "ldx < F": (dx.ptr, F - 1, n, F, dg.ptr, G, ps, pc, EINVAL),
           "x = NULL": (None, dx.ld, n, F, dg.ptr, G, ps, pc, EINVAL),
           "group = NULL": (dx.ptr, dx.ld, n, F, None, G, ps, pc, EINVAL),
           "sums = NULL": (dx.ptr, dx.ld, n, F, dg.ptr, G, None, pc, EINVAL),
           "counts = NULL": (dx.ptr, dx.ld, n, F, dg.ptr, G, ps, None, EINVAL),
           "too many workgroups": (dx.ptr, big, n, big, dg.ptr, big, ps, pc, EUNSUPPORTED)}
    for what, args in bad.items():
        rc = lib.rg_group_sums_update(*args[:-1], None)
        assert rc == args[-1], "rg_group_sums_update, %s: returned %d" % (what, rc)
        assert b"group_sums_update" in lib.rg_last_error(), what
        torch.cuda.synchronize()
        assert sums.untouched() and counts.untouched(), what
    assert lib.rg_group_sums_update(dx.ptr, dx.ld, 0, F, dg.ptr, G, ps, pc, None) == 0           # no rows: RG_OK, nothing launched
    torch.cuda.synchronize()
    assert sums.untouched() and counts.untouched()


# ------------------------------------------------------------------ rg_match_ranks
def _match(lib, a, b, target, ld_extra=0, shift=0):
    """one rg_match_ranks call -> (rank, dtarget) as numpy; target: numpy int32 or None"""
    na, F = a.shape
    da, db = RowsD(a, F + ld_extra, shift), RowsD(b, F + ld_extra, shift)
    tg = None if target is None else Ints(target, BAD_TARGET)
    rank, dt = GuardedI(na), GuardedD((na,))
    rc = lib.rg_match_ranks(da.ptr, da.ld, na, db.ptr, db.ld, b.shape[0], F, None if tg is None else tg.ptr, rank.t.data_ptr(),
                            dt.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert rank.intact() and dt.intact(), "rg_match_ranks wrote outside rank / dtarget"
    return rank.t.cpu().numpy(), dt.t.cpu().numpy()


_MATCH = {}


def _mcase(na, nb, F):
    key = (na, nb, F)
    if key not in _MATCH:
        a, b, target = integer_rows(na, nb, F, seed=1000 * F + 7 * na + nb)
        _MATCH[key] = (a, b, target) + match_ranks_ref(a, b, target)
    return _MATCH[key]


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", F_SIZES)
def test_match_ranks_every_row_count_pair(half, F):
    lib = _abi.load(half)
    for na in MATCH_ROWS:
        for nb in MATCH_ROWS:
            a, b, target, wrank, wd = _mcase(na, nb, F)
            rank, d = _match(lib, a, b, target)
            what = "%s na=%d nb=%d F=%d" % (half, na, nb, F)
            assert rank.dtype == np.int32 and np.array_equal(rank, wrank), "%s: ranks\n%r\n%r" % (what, rank, wrank)
            assert _same_bits(d, wd), what + ": dtarget"
            if nb >= 3:                                      # the planted ties: one duplicate of the target row below it, one above
                d0 = dist2_f64(a[:1], b)[0]
                assert d0[0] == d0[nb - 1] == wd[0] and wrank[0] == int((d0 < wd[0]).sum() + (d0[:nb // 2] == wd[0]).sum()) >= 1


@pytest.mark.parametrize("half", BUILDS)
def test_match_ranks_strides_null_target_and_a_long_b(half):
    lib = _abi.load(half)
    for F in (33, 70):
        a, b, target, wrank, wd = _mcase(65, 130, F)
        for ld_extra, shift in STRIDES:
            rank, d = _match(lib, a, b, target, ld_extra, shift)
            assert np.array_equal(rank, wrank) and _same_bits(d, wd), "%s F=%d ld=F+%d shift=%d" % (half, F, ld_extra, shift)
        for na, nb in ((65, 130), (130, 130), (64, 64), (1, 1)):      # target = NULL: row r's partner is row r
            a, b, _, _, _ = _mcase(na, nb, F)
            wrank, wd = match_ranks_ref(a, b, None)
            rank, d = _match(lib, a, b, None)
            assert np.array_equal(rank, wrank) and _same_bits(d, wd), "%s target = NULL na=%d nb=%d" % (half, na, nb)
        # a set against itself: every row is its own nearest row; a duplicate with a lower index goes first
        a, _, _, _, _ = _mcase(130, 130, F)
        rank, d = _match(lib, a, a, None)
        assert np.array_equal(d, np.zeros(130)) and rank[129] == 1 and np.array_equal(rank, match_ranks_ref(a, a, None)[0])
    a, b, target = integer_rows(65, 8262, 3, seed=4)           # 130 tiles of b over 128 parts: two parts walk two tiles
    wrank, wd = match_ranks_ref(a, b, target)
    rank, d = _match(lib, a, b, target)
    assert np.array_equal(rank, wrank) and _same_bits(d, wd) and wrank.max() > 64


@pytest.mark.parametrize("half", BUILDS)
def test_match_ranks_nan_rows(half):
    lib = _abi.load(half)
    a, b, target, _, _ = _mcase(65, 130, 33)
    a, b, target = a.copy(), b.copy(), target.copy()
    b[70, 5] = np.nan                                         # one NaN feature is enough
    target[3] = 70                                            # a NaN target: rank nb - 1
    a[9, :] = np.nan                                          # a NaN query row: its d* is NaN as well
    wrank, wd = match_ranks_ref(a, b, target)
    assert wrank[3] == 129 and wrank[9] == 129 and np.isnan(wd[3]) and np.isnan(wd[9])
    rank, d = _match(lib, a, b, target)
    assert np.array_equal(rank, wrank) and np.array_equal(np.isnan(d), np.isnan(wd))
    keep = ~np.isnan(wd)
    assert _same_bits(d[keep], wd[keep])
    clean = np.delete(b, 70, axis=0)                          # the NaN row of b is closer to nobody
    tclean = np.where(target > 70, target - 1, target)
    keep[3] = False
    assert np.array_equal(rank[keep], match_ranks_ref(a, clean, tclean)[0][keep])
    # a bad target is clamped, never followed outside b
    bad = target.copy()
    bad[0], bad[1] = -5, 1 << 29
    fixed = np.clip(bad, 0, 129)
    rank, d = _match(lib, a, b, bad)
    wrank, wd = match_ranks_ref(a, b, fixed)
    assert np.array_equal(rank, wrank)


_FLOATS = {}


def _floats():
    if not _FLOATS:
        rng = np.random.default_rng(78)
        a, b = rng.standard_normal((130, 70)), rng.standard_normal((130, 70))
        a[:65] = b[:65] + 0.05 * rng.standard_normal((65, 70))      # half the queries sit next to their partner: ranks 0 and large
        target = rng.permutation(130).astype(np.int32)
        target[:65] = np.arange(65)
        d = dist2_f64(a, b)
        g = GAMMA(70)
        _FLOATS.update(a=a, b=b, target=target, ref=ranks_from_d2(d, target), lo=ranks_from_d2(d, target, 1.0 - 2.0 * g)[0],
                       hi=ranks_from_d2(d, target, 1.0 + 2.0 * g)[0])
    return _FLOATS


@pytest.mark.parametrize("half", BUILDS)
def test_match_ranks_general_floats_and_graph_replay(half):
    lib = _abi.load(half)
    ref = _floats()
    a, b, target = ref["a"], ref["b"], ref["target"]
    rank, d = _match(lib, a, b, target, 5, 1)
    wrank, wd = ref["ref"]
    bound = 2.0 * GAMMA(70) * np.maximum(d, wd)
    err = np.abs(d - wd)
    print("%s: max |d* dev - ref| / (2 gamma max) = %.3g; ranks: lower %d <= device %d <= upper %d (restatement %d)" % (
        half, float((err / bound).max()), ref["lo"].sum(), rank.sum(), ref["hi"].sum(), wrank.sum()))
    assert np.isfinite(d).all() and np.all(err <= bound)
    assert np.all(ref["lo"] <= rank) and np.all(rank <= ref["hi"])
    assert (rank[:65] == 0).all() and rank[65:].max() > 10
    again = _match(lib, a, b, target, 5, 1)
    assert np.array_equal(again[0], rank) and _same_bits(again[1], d), "the same bits on every run"
    # both entry points captured on one stream into one graph, replayed once: the bits of the eager calls
    x, ids, wsums, wcounts = _case(130, 33, 7, "planted")
    dx, dg = Rows(x, 38, 1), Ints(ids, 0)
    da, db, tg = RowsD(a, 75, 1), RowsD(b, 70), Ints(target, BAD_TARGET)
    sums, counts, grank, gd = GuardedD((7, 33)), GuardedL(7), GuardedI(130), GuardedD((130,))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.rg_group_sums_update(dx.ptr, dx.ld, 130, 33, dg.ptr, 7, sums.t.data_ptr(), counts.t.data_ptr(), st) == 0, lib.rg_last_error()
        assert lib.rg_match_ranks(da.ptr, da.ld, 130, db.ptr, db.ld, 130, 70, tg.ptr, grank.t.data_ptr(), gd.t.data_ptr(), st) == 0, \
            lib.rg_last_error()
    sums.t.zero_(); counts.t.zero_(); grank.t.fill_(SBITS); gd.t.fill_(DSENT)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(sums.t.cpu().numpy(), wsums) and np.array_equal(counts.t.cpu().numpy(), wcounts)
    assert np.array_equal(grank.t.cpu().numpy(), rank) and _same_bits(gd.t.cpu().numpy(), d)
    assert sums.intact() and counts.intact() and grank.intact() and gd.intact()


@pytest.mark.parametrize("half", BUILDS)
@pytest.mark.parametrize("F", [33, 70])
def test_float_and_double_distance_paths_hold_the_same_bits(half, F):
    """d2(a_r, b_t) as rg_radius_hits states it (fp32 rows, 32 features per pass: its mind2 against the ONE row b_t) equals, under
    == on the int64 views, d2 as rg_match_ranks states it (the rows widened to fp64, 16 features per pass: its dtarget with
    target = t everywhere).  70 and 67 rows straddle the 64-row tile, F = 33 and 70 one fp32 pass and the fp64 passes."""
    lib = _abi.load(half)
    a, b = wide_floats(70, F, seed=300 + F), wide_floats(67, F, seed=400 + F)
    da, db = Rows(a, F + 5, 1), Rows(b, F + 3)
    wa, wb = RowsD(a, F + 2), RowsD(b, F + 1, 1)               # np.float64(fp32 value): exact
    need = lib.rg_pairdist_ws_bytes(70, 1, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for t in (0, 63, 64, 66):
        mind2, rank, dt, tg = GuardedD((70,)), GuardedI(70), GuardedD((70,)), Ints(np.full(70, t), BAD_TARGET)
        rc = lib.rg_radius_hits(da.ptr, da.ld, 70, db.ptr + 4 * t * db.ld, db.ld, 1, F, None, ws.data_ptr(), need, None,
                                mind2.t.data_ptr(), None)
        assert rc == 0, lib.rg_last_error()
        rc = lib.rg_match_ranks(wa.ptr, wa.ld, 70, wb.ptr, wb.ld, 67, F, tg.ptr, rank.t.data_ptr(), dt.t.data_ptr(), None)
        assert rc == 0, lib.rg_last_error()
        torch.cuda.synchronize()
        assert mind2.intact() and rank.intact() and dt.intact()
        f32, f64 = mind2.t.cpu().numpy(), dt.t.cpu().numpy()
        assert np.isfinite(f32).all() and (f32 > 0).all(), "%s F=%d t=%d: a row or column past the operand was read" % (half, F, t)
        assert np.array_equal(f32.view(np.int64), f64.view(np.int64)), "%s F=%d t=%d: the fp32 and the fp64 path differ" % (half, F, t)


@pytest.mark.parametrize("half", BUILDS)
def test_match_ranks_rejected_arguments_write_nothing(half):
    lib = _abi.load(half)
    na, nb, F = 70, 5, 17
    a, b, target, _, _ = _mcase(na, nb, F)
    da, db, tg = RowsD(a, F + 2), RowsD(b, F + 1), Ints(target, BAD_TARGET)
    rank, dt = GuardedI(na), GuardedD((na,))
    pr, pd = rank.t.data_ptr(), dt.t.data_ptr()
    #             a       lda    na  b       ldb    nb  F  target  rank dtarget
    bad = {"F = 0": (da.ptr, da.ld, na, db.ptr, db.ld, nb, 0, tg.ptr, pr, pd),
           "nb = 0": (da.ptr, da.ld, na, db.ptr, db.ld, 0, F, tg.ptr, pr, pd),
           "nb < 0": (da.ptr, da.ld, na, db.ptr, db.ld, -1, F, tg.ptr, pr, pd),
           "na < 0": (da.ptr, da.ld, -1, db.ptr, db.ld, nb, F, tg.ptr, pr, pd),
           "lda < F": (da.ptr, F - 1, na, db.ptr, db.ld, nb, F, tg.ptr, pr, pd),
           "ldb < F": (da.ptr, da.ld, na, db.ptr, F - 1, nb, F, tg.ptr, pr, pd),
           "a = NULL": (None, da.ld, na, db.ptr, db.ld, nb, F, tg.ptr, pr, pd),
           "b = NULL": (da.ptr, da.ld, na, None, db.ld, nb, F, tg.ptr, pr, pd),
           "rank = NULL": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, tg.ptr, None, pd),
           "dtarget = NULL": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, tg.ptr, pr, None),
           "target = NULL with na > nb": (da.ptr, da.ld, na, db.ptr, db.ld, nb, F, None, pr, pd)}
    for what, args in bad.items():
        rc = lib.rg_match_ranks(*args, None)
        assert rc == EINVAL, "rg_match_ranks, %s: returned %d" % (what, rc)
        assert b"match_ranks" in lib.rg_last_error(), what
        torch.cuda.synchronize()
        assert rank.untouched() and dt.untouched(), what
    assert lib.rg_match_ranks(da.ptr, da.ld, 0, db.ptr, db.ld, nb, F, tg.ptr, pr, pd, None) == 0       # no query rows: nothing written
    torch.cuda.synchronize()
    assert rank.untouched() and dt.untouched()
