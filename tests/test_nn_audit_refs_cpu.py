"""The numpy restatements of tests/nn_audit_refs.py against brute-force Python, the audit's host arithmetic on hand-built distance
lists, the CPU-tensor path of rna_gan_amd.nearest against the restatements, MemoryError before allocation, and the CLI's refusal of
--mem_samples without --resident 1.  No GPU."""
import pickle

import numpy as np
import pytest
import torch

import nn_audit_refs as R


def _tiles(seed, N, C, S):
    return np.random.default_rng(seed).integers(0, 256, size=(N, C, S, S), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("C,S,f", [(3, 8, 1), (3, 8, 2), (1, 16, 4), (2, 8, 8)])
def test_descriptor_restatement_against_python_loops(C, S, f):
    t = _tiles(C * 100 + S + f, 2, C, S)
    desc, norm2 = R.descriptor(t, f)
    P = S // f
    D = C * P * P
    assert desc.shape == (2, R.ldd_of(D)) and desc.dtype == np.int8 and norm2.dtype == np.int32
    for n in range(2):
        want = []
        for c in range(C):
            for y in range(P):
                for x in range(P):
                    s = sum(int(t[n, c, y * f + dy, x * f + dx]) for dy in range(f) for dx in range(f))
                    want.append((s + f * f // 2) // (f * f) - 128)
        assert desc[n, :D].tolist() == want
        assert not desc[n, D:].any()
        assert int(norm2[n]) == sum(v * v for v in want)


def test_descriptor_extremes_and_the_rounding_tie():
    t = np.zeros((1, 1, 4, 4), np.uint8)
    t[0, 0, :2, 2:] = 255
    t[0, 0, 2:, :2] = [[1, 1], [0, 0]]            # block sum 2 = f f / 2: the tie rounds up
    t[0, 0, 2:, 2:] = [[1, 0], [0, 0]]            # block sum 1: rounds down
    desc, norm2 = R.descriptor(t, 2)
    assert desc[0, :4].tolist() == [-128, 127, -127, -128]
    assert int(norm2[0]) == 128 * 128 * 2 + 127 * 127 * 2


def test_topk_restatement_against_python():
    rng = np.random.default_rng(3)
    a = rng.integers(-128, 128, size=(5, 64), dtype=np.int8)
    b = rng.integers(-128, 128, size=(11, 64), dtype=np.int8)
    b[7] = b[2]                                   # a tie in every query: the lower row first
    excl = [2, -1, 11, 0, 7]
    for k, exclude in ((1, None), (4, None), (3, excl)):
        keys = R.topk_keys(a, R.norms(a), b, R.norms(b), 64, k, exclude)
        for q in range(5):
            cand = []
            for r in range(11):
                if exclude is not None and r == exclude[q]:
                    continue
                d2 = sum((int(x) - int(y)) ** 2 for x, y in zip(a[q], b[r]))
                cand.append((d2, r))
            cand.sort()
            assert [(int(key) >> 32, int(key) & 0xffffffff) for key in keys[q]] == cand[:k]
    d2, ix = R.split_keys(R.topk_keys(b[2:3], R.norms(b[2:3]), b, R.norms(b), 64, 2))
    assert d2.tolist() == [[0, 0]] and ix.tolist() == [[2, 7]]


def test_topk_restatement_ignores_columns_beyond_D():
    rng = np.random.default_rng(4)
    a = rng.integers(-128, 128, size=(3, 128), dtype=np.int8)
    b = rng.integers(-128, 128, size=(6, 128), dtype=np.int8)
    na, nb = R.norms(a[:, :64]), R.norms(b[:, :64])
    want = R.topk_keys(a[:, :64], na, b[:, :64], nb, 64, 2)
    assert np.array_equal(R.topk_keys(a, na, b, nb, 64, 2), want)


# ---------------------------------------------------------------------------------------------- host arithmetic
def test_copied_copy_rate_and_heldout_statistic_by_hand():
    from rna_gan_amd import nearest as NN
    # sample 0 copies (5 < 9); 1 ties with the leave-one-out distance (no copy); 2 is far; 3 copies one of an exact duplicate pair
    # (loo 0: never flagged, but exact); 4 is exact on a tile with no duplicate
    d2 = np.array([[5, 40], [9, 12], [70, 71], [0, 0], [0, 3]], np.int64)
    loo = np.array([9, 9, 30, 0, 8], np.int64)
    assert NN.copied_flags(d2[:, 0], loo).tolist() == [True, False, False, False, True]
    assert R.copied(d2[:, 0], loo).tolist() == [True, False, False, False, True]
    res = NN.AuditResult(d2, np.zeros_like(d2), loo, heldout_d2=np.array([9, 9, 100, 0], np.int64))
    assert res.copy_rate == 2 / 5 and res.exact.tolist() == [False, False, False, True, True] and res.exact_rate == 2 / 5
    # pairs with d_g < d_h: 5 -> 3, 9 -> 1, 70 -> 1, 0 -> 3, 0 -> 3 = 11; ties: 9 -> 2, 0 -> 1, 0 -> 1 = 4
    assert res.closer_than_heldout == (11 + 2.0) / 20
    assert R.closer_than_heldout(d2[:, 0].tolist(), [9, 9, 100, 0]) == (11 + 2.0) / 20
    assert NN.closer_than_heldout([3, 3], [3, 3, 3]) == 0.5
    assert NN.closer_than_heldout([1], [2, 3]) == 1.0 and NN.closer_than_heldout([4], [2, 3]) == 0.0
    s = res.summary()
    assert s["min_d2"] == 0 and s["median_d2"] == 5.0 and s["copy_rate"] == 0.4 and s["exact"] == 0.4
    assert NN.AuditResult(d2, np.zeros_like(d2), loo).closer_than_heldout is None
    rng = np.random.default_rng(0)
    dg, dh = rng.integers(0, 20, 40), rng.integers(0, 20, 30)
    assert NN.closer_than_heldout(dg, dh) == pytest.approx(R.closer_than_heldout(dg.tolist(), dh.tolist()), abs=1e-15)


def test_merge_symmetries_counts_a_row_once_at_its_smallest_distance():
    from rna_gan_amd import nearest as NN
    d_a, i_a = np.array([[4, 9, 9]]), np.array([[7, 1, 3]])
    d_b, i_b = np.array([[2, 6, 9]]), np.array([[3, 7, 0]])
    d, i = NN.merge_symmetries([d_a, d_b], [i_a, i_b], 3)
    assert d.tolist() == [[2, 4, 9]] and i.tolist() == [[3, 7, 0]]


# ---------------------------------------------------------------------------------------------- the CPU-tensor path
@pytest.mark.parametrize("C,S,f", [(3, 8, 1), (3, 8, 2), (1, 16, 4), (3, 64, 8), (3, 32, 32)])
def test_cpu_descriptors_equal_the_restatement(C, S, f):
    from rna_gan_amd import nearest as NN
    t = _tiles(S + f, 3, C, S)
    t[0, 0] = 0
    t[1, -1] = 255
    desc, norm2 = NN.descriptors(torch.from_numpy(t), f)
    wd, wn = R.descriptor(t, f)
    assert desc.dtype == torch.int8 and norm2.dtype == torch.int32
    assert np.array_equal(desc.numpy(), wd) and np.array_equal(norm2.numpy(), wn)


def test_cpu_nearest_equals_the_restatement():
    from rna_gan_amd import nearest as NN
    rng = np.random.default_rng(8)
    a = rng.integers(-128, 128, size=(17, 128), dtype=np.int8)
    b = rng.integers(-128, 128, size=(300, 128), dtype=np.int8)
    b[200] = b[5]
    a[0] = b[5]
    excl = np.full(17, -1, np.int32)
    excl[0], excl[1], excl[2] = 5, 300, 12
    for k, e in ((1, None), (8, None), (4, excl)):
        d2, ix = NN.nearest((torch.from_numpy(a), torch.from_numpy(R.norms(a))), torch.from_numpy(b), k,
                            None if e is None else torch.from_numpy(e))
        wd, wi = R.split_keys(R.topk_keys(a, R.norms(a), b, R.norms(b), 128, k, e))
        assert d2.dtype == torch.int64 and np.array_equal(d2.numpy(), wd) and np.array_equal(ix.numpy(), wi)
    d2, ix = NN.nearest(torch.from_numpy(a[:1]), torch.from_numpy(b), 2)
    assert d2.tolist() == [[0, 0]] and ix.tolist() == [[5, 200]]
    with pytest.raises(ValueError):
        NN.nearest(torch.from_numpy(a), torch.from_numpy(b[:4]), 4, torch.from_numpy(excl))
    with pytest.raises(ValueError):
        NN.nearest(torch.from_numpy(a), torch.from_numpy(b), 9)
    d2, ix = NN.nearest(torch.from_numpy(a[:0]), torch.from_numpy(b), 3)
    assert tuple(d2.shape) == (0, 3) and tuple(ix.shape) == (0, 3)


def _audit_case():
    """24 training tiles 3 x 16 x 16 with an exact duplicate pair (3, 19); generated: a noisy copy of 7, of 11 rotated, of 3 (one of
    the pair), an exact copy of 5, and two fresh tiles.

    A sample drawn from the training distribution itself is flagged about half of the time (its distance to the nearest training
    tile and that tile's to its own neighbour are two draws of one distribution), so what must NOT be flagged is built to be
    farther away than training tiles are from each other: the training bytes are uniform in [64, 192) (2 var = 2 731 per byte
    between two of them), the fresh tiles uniform in [0, 256) (5 461 + 1 365 = 6 826 to a training tile), and tile 11 carries a
    left / right step of +-60 that no other tile has, so that its quarter turn differs from every tile by at least that step's
    3 600 per byte on top."""
    rng = np.random.default_rng(21)
    train = rng.integers(64, 192, size=(24, 3, 16, 16), dtype=np.uint8)
    train[11, :, :, :8] += 60
    train[11, :, :, 8:] -= 60
    train[19] = train[3]

    def noisy(t):
        return np.clip(t.astype(np.int16) + rng.integers(-1, 2, size=t.shape), 0, 255).astype(np.uint8)
    gen = np.stack([noisy(train[7]), R.d4(noisy(train[11]), 1), noisy(train[3]), train[5].copy(),
                    rng.integers(0, 256, size=(3, 16, 16), dtype=np.uint8), rng.integers(0, 256, size=(3, 16, 16), dtype=np.uint8)])
    held = rng.integers(64, 192, size=(5, 3, 16, 16), dtype=np.uint8)
    return train, gen, held


@pytest.mark.parametrize("d4", [False, True])
def test_cpu_audit_equals_the_restatement(d4):
    from rna_gan_amd import nearest as NN
    train, gen, held = _audit_case()
    index = NN.TrainIndex(torch.from_numpy(train), factor=2, chunk=7)
    res = NN.audit(torch.from_numpy(gen), index, k=3, d4=d4, heldout_u8=torch.from_numpy(held))
    want = R.audit(gen, train, 2, 3, d4, held)
    for name in ("d2", "index", "loo_d2", "copied", "exact"):
        assert np.array_equal(getattr(res, name), want[name]), name
    assert res.copy_rate == want["copy_rate"] and res.closer_than_heldout == want["closer_than_heldout"]
    # the noisy copy of 7 and the exact copy of 5 are flagged; the rotated one only under d4; the copy of the duplicated tile never
    # (loo_d2 = 0); no fresh tile
    assert res.copied.tolist() == [True, d4, False, True, False, False]
    assert res.index[[0, 3], 0].tolist() == [7, 5] and res.index[2, 0] in (3, 19) and res.loo_d2[2] == 0
    assert res.exact.tolist() == [False, False, False, True, False, False]
    if d4:
        assert res.index[1, 0] == 11


def test_train_index_refuses_before_allocating(monkeypatch):
    from rna_gan_amd import nearest as NN
    t = torch.zeros((10, 3, 16, 16), dtype=torch.uint8)
    need = 10 * 192 + 10 * 4                      # D = 3 * 8 * 8 = 192 = ldd at factor 2
    index = NN.TrainIndex(t, factor=2, max_bytes=need)
    assert index.ldd == 192 and len(index) == 10 and int(index.norm2[0]) == 192 * 128 * 128

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the budget was checked")
    monkeypatch.setattr(NN.torch, "empty", no_alloc)
    with pytest.raises(MemoryError):
        NN.TrainIndex(t, factor=2, max_bytes=need - 1)
    with pytest.raises(ValueError):
        NN.TrainIndex(torch.zeros((1, 3, 256, 256), dtype=torch.uint8), factor=1)        # D = 196 608 > 32 768


# ---------------------------------------------------------------------------------------------- metric settings and the CLI
def test_metric_pickle_keeps_settings_and_history_only():
    from rna_gan_amd.metrics import Memorisation
    m = Memorisation(torch.zeros((4, 3, 8, 8), dtype=torch.uint8), 6, factor=2, k=2, d4=True, encoding_dims=5, seed=3)
    m.history.append({"copy_rate": 0.5, "exact": 0.0, "min_d2": 3, "median_d2": 8.0})
    m._index = object()
    back = pickle.loads(pickle.dumps(m))
    assert (back.n_fake, back.factor, back.k, back.d4, back.seed) == (6, 2, 2, True, 3)
    assert back.history == m.history and back.train_tiles is None and back._index is None and back.noise is None
    with pytest.raises(RuntimeError):
        back.metric_ops(None, "cpu")
    for bad in ({"factor": 3}, {"k": 0}, {"k": 9}):
        with pytest.raises(ValueError):
            Memorisation(None, 4, **bad)


def test_cli_refuses_mem_samples_without_resident(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json"]
    a = H.parse_args(base)
    assert (a.mem_samples, a.mem_factor, a.mem_d4) == (0, 4, 1)
    a = H.parse_args(base + ["--resident", "1", "--mem_samples", "64", "--mem_factor", "8", "--mem_d4", "0"])
    assert (a.mem_samples, a.mem_factor, a.mem_d4) == (64, 8, 0)
    with pytest.raises(SystemExit):
        H.parse_args(base + ["--mem_samples", "64"])
    assert "--mem_samples needs --resident 1" in capsys.readouterr().err
    for bad in (["--mem_samples", "-1"], ["--mem_factor", "3"], ["--mem_d4", "2"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + ["--resident", "1"] + bad)
    capsys.readouterr()
