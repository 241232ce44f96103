"""rg_rows_gather_f32 (include/rnagan_hip.h) through ctypes on both builds of the library, bit for bit against the plain loops of
tests/rna_table_refs.py (pinned without a GPU by tests/test_rna_tables_cpu.py).

The destination lives inside a SENTINEL-filled allocation (a write outside dst[0 .. N)[0 .. ld_dst) changes the pattern).  The
table -- finite values -- lives inside an allocation filled with NaN, and so do the columns [F, ld_table) of its own rows: a read
outside table[0 .. M)[0 .. F) makes a result NaN.  Such overruns stay inside the allocations, so nothing can fault -- the
out-of-range indices of the clamp test included: the kernel's contract is to read the nearest valid row, and were it broken for
-1 or M the read would land in the NaN surroundings (sized to hold a whole row on either side); the +-2^31 cases are sent only
with the ones before them verified in the same process.

Both bases are moved 0, 4, 8 and 12 bytes off a 16-byte boundary, independently: with the row strides F, F + 1, F + 3 and
ceil64(F) every (source row, destination row) pair of relative alignments occurs -- 16-, 8- and 4-byte loads, head chunks of
one to three floats, tails, and rows shorter than one chunk."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rna_gan_amd import _abi
from both_builds import fp16_twin
from guarded import Guarded, SBITS
from rna_table_refs import rows_gather_ref
from vae_fid_refs import SENTINEL, bits, ceil64

FS = [1, 2, 3, 5, 64, 130, 19198]
BUILDS = {torch.bfloat16: "bf16", torch.float16: "f16"}
OFFS = (0, 1, 2, 3)                      # floats off a 16-byte boundary: 0, 4, 8, 12 bytes
_DATA, _WANT = {}, {}


def _table(M, F):
    """The table's data as numpy, computed once per shape and never modified."""
    key = (M, F)
    if key not in _DATA:
        a = np.random.default_rng([43, M, F]).normal(size=(M, F)).astype(np.float32)
        a[0, 0] = -0.0                                             # bits travel, not values
        a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def _index(M, N, seed=0):
    """N indices into M rows: a permutation's start, then repeats (the first index again, and one row three times)."""
    idx = np.random.default_rng([47, M, N, seed]).permutation(M)[:N].tolist()
    while len(idx) < N:
        idx.append(idx[0] if len(idx) % 2 else M - 1)
    if N >= 3:
        idx[-1] = idx[-2] = idx[0]
    return idx


def _want(M, F, index, ld_dst, clamped=None):
    """The loops' result on the device, computed once per case (the loops run once per (table, index); the pad is zeros)."""
    key = (M, F, tuple(index), ld_dst)
    if key not in _WANT:
        core = (M, F, tuple(index))
        if core not in _WANT:
            _WANT[core] = rows_gather_ref(_table(M, F), F, index if clamped is None else clamped)
        full = np.zeros((len(index), ld_dst), dtype=np.float32)
        full[:, :F] = _WANT[core]
        full.view(np.uint32)[:, :F] = _WANT[core].view(np.uint32)
        _WANT[key] = torch.from_numpy(full).cuda()
    return _WANT[key]


def _src(M, F, ld_table, toff):
    """The table on the device at row stride ld_table, its base toff floats off a 16-byte boundary, NaN everywhere else."""
    host = np.full((M, ld_table), np.nan, dtype=np.float32)
    host[:, :F] = _table(M, F)
    host.view(np.uint32)[:, :F] = _table(M, F).view(np.uint32)
    pad = (ld_table + 63) // 64 * 64 + 64                          # a whole row in front of and behind the table
    return Guarded(torch.from_numpy(host), float("nan"), before=pad + toff, after=pad)


def _launch(lib, src, M, F, ld_table, dindex, dst, N, ld_dst, stream=None):
    return lib.rg_rows_gather_f32(src.t.data_ptr(), M, F, ld_table, None if dindex is None else dindex.data_ptr(),
                                  dst.t.data_ptr(), N, ld_dst, None if stream is None else stream.cuda_stream)


def _run(lib, M, F, index, n=None, ld_table=None, ld_dst=None, toff=0, doff=0, stream=None, src=None, dindex=None, want=None,
         clamped=None):
    """One launch inside guarded allocations, compared with the loops on the device."""
    ld_table = F if ld_table is None else ld_table
    ld_dst = F if ld_dst is None else ld_dst
    N = n if index is None else len(index)
    src = _src(M, F, ld_table, toff) if src is None else src
    dst = Guarded(torch.full((N, ld_dst), SENTINEL, dtype=torch.float32), SENTINEL, before=128 + doff, after=4096)
    assert src.t.data_ptr() % 16 == 4 * toff and dst.t.data_ptr() % 16 == 4 * doff
    if dindex is None and index is not None:
        dindex = torch.tensor(index, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = _launch(lib, src, M, F, ld_table, dindex, dst, N, ld_dst, stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert dst.surroundings_keep(SBITS), "rg_rows_gather_f32 wrote outside dst"
    if want is None:
        want = _want(M, F, list(range(N)) if index is None else index, ld_dst, clamped)
    if not torch.equal(bits(dst.t), bits(want)):
        got, w = dst.t.cpu().numpy(), want.cpu().numpy()
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != w.view(np.uint32).reshape(-1))
        raise AssertionError("M %d F %d N %d ld_table %d ld_dst %d offsets %d / %d: %d of %d elements differ, first at flat index "
                             "%d: got %r want %r" % (M, F, N, ld_table, ld_dst, toff, doff, bad.size, w.size, bad[0],
                                                     got.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]]))
    return dst


@fp16_twin
@pytest.mark.parametrize("F", FS)
def test_bit_exact(F, h16=torch.bfloat16):
    """M in {1, 7} x N in {1, 9} x ld_table in {F, F + 3} x ld_dst in {F, ceil64(F), F + 1} x 4 x 4 base offsets: repeated and
    permuted indices, the pad columns demanded zero."""
    lib = _abi.load(BUILDS[h16])
    for M in (1, 7):
        for ld_table in (F, F + 3):
            for toff in OFFS:
                src = _src(M, F, ld_table, toff)
                for N in (1, 9):
                    index = _index(M, N)
                    dindex = torch.tensor(index, dtype=torch.int32, device="cuda")
                    for ld_dst in sorted({F, ceil64(F), F + 1}):
                        for doff in OFFS:
                            _run(lib, M, F, index, ld_table=ld_table, ld_dst=ld_dst, toff=toff, doff=doff, src=src, dindex=dindex)
    assert not bool(torch.isnan(_want(7, F, _index(7, 9), F)).any())


@pytest.mark.parametrize("F", [3, 130, 19198])
def test_reversed_and_permuted_indices(F):
    lib = _abi.load()
    M = 7
    for index in (list(range(M - 1, -1, -1)), np.random.default_rng(53).permutation(M).tolist(), [M - 1] * 5, [0, 0, 0]):
        _run(lib, M, F, index, ld_table=F + 3, ld_dst=F + 1, toff=1, doff=2)


@pytest.mark.parametrize("F", [2, 64, 19198])
def test_null_index_is_a_plain_copy(F):
    lib = _abi.load()
    for M, N in ((7, 7), (7, 4), (1, 1)):
        dst = _run(lib, M, F, None, n=N, ld_table=F + 3, ld_dst=F, toff=3, doff=1)
        assert torch.equal(bits(dst.t), bits(torch.from_numpy(_table(M, F)[:N].copy()).cuda()))


def test_out_of_range_indices_are_clamped():
    lib = _abi.load()
    for F in (5, 130):
        M = 7
        near = [-1, 7, 3, -5, 8]
        _run(lib, M, F, near, ld_table=F + 3, ld_dst=F + 1, toff=2, clamped=[0, 6, 3, 0, 6])
        far = [-2 ** 31, 2 ** 31 - 1, 3, -(2 ** 31 - 1), 1 << 24, -(1 << 24)]
        _run(lib, M, F, far, ld_table=F + 3, ld_dst=F + 1, toff=2, clamped=[0, 6, 3, 0, 6, 0])
    _run(lib, 1, 3, [5, -5, 0], clamped=[0, 0, 0])


def test_refused_arguments_and_empty_batch():
    lib = _abi.load()
    M, F = 4, 6
    src = _src(M, F, F, 0)
    dst = Guarded(torch.full((5, 8), SENTINEL, dtype=torch.float32), SENTINEL)
    index = torch.zeros(5, dtype=torch.int32, device="cuda")
    t, d, x = src.t.data_ptr(), dst.t.data_ptr(), index.data_ptr()
    #       table M  F  ld_table index dst N ld_dst
    bad = [(None, M, F, F, x, d, 2, 8), (t, M, F, F, x, None, 2, 8), (t, 0, F, F, x, d, 2, 8), (t, -1, F, F, x, d, 2, 8),
           (t, M, F, F, x, d, -1, 8), (t, M, 0, F, x, d, 2, 8), (t, M, -F, F, x, d, 2, 8), (t, M, F, F - 1, x, d, 2, 8),
           (t, M, F, F, x, d, 2, F - 1), (t, M, F, F, None, d, 5, 8), (t, M, F, 0, x, d, 2, 8), (t, M, F, F, x, d, 2, 0)]
    for args in bad:
        assert lib.rg_rows_gather_f32(*args, None) == -1, args                    # RG_EINVAL
        assert lib.rg_last_error()
    assert lib.rg_rows_gather_f32(t, M, F, F, x, d, 0, 8, None) == 0             # N == 0: RG_OK, nothing launched
    assert lib.rg_rows_gather_f32(t, 0, F, F, None, d, 0, 8, None) == 0          # ... an empty table included
    torch.cuda.synchronize()
    assert bool((bits(dst.flat) == SBITS).all()), "a refused or empty call wrote"
    assert lib.rg_rows_gather_f32(t, M, F, F, x, d, 5, 8, None) == 0             # N > M is fine WITH an index
    assert lib.rg_rows_gather_f32(t, M, F, F, None, d, 4, 8, None) == 0          # N == M without one
    torch.cuda.synchronize()
    assert dst.surroundings_keep(SBITS)


def test_non_default_stream():
    lib = _abi.load()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _run(lib, 7, 130, _index(7, 9, seed=2), ld_table=133, ld_dst=192, toff=1, doff=3, stream=side)


def test_twice_into_the_same_destination():
    lib = _abi.load()
    M, F = 7, 130
    a, b = _index(M, 9, seed=3), _index(M, 9, seed=4)
    assert a != b
    dst = _run(lib, M, F, a, ld_dst=F + 1, doff=1)
    src = _src(M, F, F, 0)
    db = torch.tensor(b, dtype=torch.int32, device="cuda")
    assert _launch(lib, src, M, F, F, db, dst, 9, F + 1) == 0
    torch.cuda.synchronize()
    assert dst.surroundings_keep(SBITS) and torch.equal(bits(dst.t), bits(_want(M, F, b, F + 1)))


def test_graph_replay_equals_eager():
    lib = _abi.load()
    M, F, N, ld = 7, 19198, 9, ceil64(19198)
    index = _index(M, N, seed=5)
    src = _src(M, F, F, 2)
    dindex = torch.tensor(index, dtype=torch.int32, device="cuda")
    eager = _run(lib, M, F, index, ld_dst=ld, toff=2, src=src, dindex=dindex).t.clone()
    dst = Guarded(torch.full((N, ld), SENTINEL, dtype=torch.float32), SENTINEL)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rc = _launch(lib, src, M, F, F, dindex, dst, N, ld, torch.cuda.current_stream())
    assert rc == 0, lib.rg_last_error()
    for other in (_index(M, N, seed=6), index):                     # the replay reads the index buffer as it is NOW
        dindex.copy_(torch.tensor(other, dtype=torch.int32))
        dst.t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert dst.surroundings_keep(SBITS) and torch.equal(bits(dst.t), bits(_want(M, F, other, ld)))
    assert torch.equal(bits(dst.t), bits(eager))


def test_python_wrapper():
    from rna_gan_amd.rna_tables import rows_gather
    M, F = 7, 130
    rows = torch.from_numpy(_table(M, F).copy()).cuda()
    index = _index(M, 9, seed=7)
    got = rows_gather(rows, torch.tensor(index, dtype=torch.int32, device="cuda"))
    assert torch.equal(bits(got), bits(_want(M, F, index, F)))
    assert torch.equal(bits(rows_gather(rows, None, n=4, ld_dst=192)), bits(_want(M, F, [0, 1, 2, 3], 192)))
    assert tuple(rows_gather(rows, None, n=0).shape) == (0, F)
    with pytest.raises(RuntimeError):
        rows_gather(rows, None, n=M + 1)                            # no index and N > M: the library refuses, the wrapper raises
    with pytest.raises(ValueError):
        rows_gather(rows, torch.zeros(3, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("log2_rows", [26, 27])
def test_offsets_are_64_bit(log2_rows):
    """ld_table = 16, F = 13, M = 2^26 + 8: a REAL allocation of 4 GiB + 512 B, filled with NaN, with distinct rows written at
    indices 0, 2^25, 2^26 - 1, 2^26 and 2^26 + 7.  A BYTE offset computed in 32 bits wraps at row 2^26 and reads NaN or a wrong
    row INSIDE the buffer -- a failed assertion, never a fault.  M = 2^27 + 8 (8 GiB + 512 B) does the same for an ELEMENT offset
    computed in a signed 32-bit int, which passes 2^31 at row 2^27.  Skips only when the device reports less than 6 GiB (11 GiB)
    free."""
    R = 1 << log2_rows
    if torch.cuda.mem_get_info()[0] < (6 << 30 if log2_rows == 26 else 11 << 30):
        pytest.skip("too little device memory free")
    lib = _abi.load()
    ld, F, M = 16, 13, R + 8
    buf = torch.full((M * ld,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.numel() * 4 == R * 64 + 512
    where = [0, R >> 1, R - 1, R, R + 7]
    small = np.random.default_rng(59).normal(size=(len(where), F)).astype(np.float32)
    for k, t in enumerate(where):
        buf[t * ld:t * ld + F] = torch.from_numpy(small[k]).cuda()
    pick = [4, 3, 2, 1, 0, 3, 4]
    dindex = torch.tensor([where[k] for k in pick], dtype=torch.int32, device="cuda")
    dst = Guarded(torch.full((len(pick), F + 1), SENTINEL, dtype=torch.float32), SENTINEL, before=129)
    torch.cuda.synchronize()
    rc = lib.rg_rows_gather_f32(buf.data_ptr(), M, F, ld, dindex.data_ptr(), dst.t.data_ptr(), len(pick), F + 1, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rg_last_error()
    assert dst.surroundings_keep(SBITS)
    got = dst.t.cpu().numpy()
    del buf
    torch.cuda.empty_cache()                         # the 4 GiB go back to the device, not into the caching allocator
    want = np.zeros((len(pick), F + 1), dtype=np.float32)
    want[:, :F] = rows_gather_ref(small, F, pick)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
