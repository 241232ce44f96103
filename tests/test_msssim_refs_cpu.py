"""tests/msssim_refs.py pinned without a GPU: against a brute-force evaluation in exact rationals, against scipy's filter and
against closed forms; the host half of rna_gan_amd.msssim (taps, default S, weights, the pair draw, the finishing) against the
same restatement; the metric's pickle and the CLI's parsing.  It also asserts what the GPU file relies on for its final-score
comparison: on the correlated inputs every per-level CS of the restatement is at least CS_FLOOR, so no pair sits near the clamp."""
import pickle

import numpy as np
import pytest

import msssim_refs as R
from rna_gan_amd import msssim as MS


@pytest.mark.parametrize("H,W,S", [(11, 11, 1), (12, 13, 1), (22, 23, 2)])
def test_restatement_equals_exact_rationals(H, W, S):
    a, b = R.correlated_sets(1, H, W, 16, seed=3)
    want = R.components_exact(a[0], b[0], S)
    got = R.components(a[0], b[0], S)
    err = np.abs(got - want).max()
    print("%d x %d S %d: restatement against exact rationals, worst %.3g" % (H, W, S, err))
    assert got.shape == (S, 2) and err < 1e-12
    u = R.random_tiles(2, H, W, 5)                                 # independent noise: CS near 0, of either sign
    assert np.abs(R.components(u[0], u[1], S) - R.components_exact(u[0], u[1], S)).max() < 1e-12


def test_window_equals_scipy_correlate1d():
    from scipy.ndimage import correlate1d
    x = R.random_tiles(1, 37, 29, 1)[0].astype(np.float64)
    g = R.taps()
    full = correlate1d(correlate1d(x, g, axis=1, mode="constant"), g, axis=0, mode="constant")
    assert np.abs(R.window(x) - full[5:-5, 5:-5]).max() < 1e-11
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.shape == (11,)
    assert np.array_equal(MS.taps(), g)


def test_pyramid_is_the_exact_block_mean():
    x = R.random_tiles(1, 45, 47, 2)[0]
    for s, p in enumerate(R.pyramid(x, 3)):
        h, w = 45 >> s, 47 >> s
        blocks = x[:h << s, :w << s].astype(np.int64).reshape(h, 1 << s, w, 1 << s, 3).sum(axis=(1, 3))
        assert p.shape == (h, w, 3) and np.array_equal(p * 4 ** s, blocks)


@pytest.mark.parametrize("H,W", [(11, 11), (23, 25), (64, 64), (177, 191)])
def test_closed_forms(H, W):
    S = R.default_scales(H, W)
    x = R.random_tiles(1, H, W, 7)[0]
    same = R.components(x, x)
    assert same.shape == (S, 2) and np.abs(same - 1.0).max() < 1e-12 and abs(R.ms_ssim(x, x) - 1.0) < 1e-12
    for c1, c2 in ((0, 255), (255, 0), (17, 200), (128, 128), (0, 0)):
        a, b = np.full((H, W, 3), c1, np.uint8), np.full((H, W, 3), c2, np.uint8)
        comp = R.components(a, b)
        l = (2.0 * c1 * c2 + R.C1) / (c1 * c1 + c2 * c2 + R.C1)
        assert np.abs(comp[:, 0] - 1.0).max() < 1e-9 and np.abs(comp[:, 1] - l).max() < 1e-9, (c1, c2, comp)
    x = R.two_scale_tile(H, W, 7)
    comp = R.components(x, 255 - x)
    assert (comp[:, 0] < 0).all() and R.ms_ssim(x, 255 - x) == 0.0, comp


@pytest.mark.parametrize("H,W", R.CORRELATED_SHAPES)
def test_correlated_inputs_keep_every_cs_above_the_floor(H, W):
    """what lets tests/test_msssim_ops_gpu.py hold the FINAL score of every correlated pair to 1e-9: the power 0.0448 of a value
    near the clamp is ill-conditioned, and these inputs never get near it"""
    worst = 1.0
    for sd in R.SDS:
        a, b = R.correlated_sets(2, H, W, sd)
        for k in range(2):
            comp = R.components(a[k], b[k])
            worst = min(worst, comp[:, 0].min())
            assert comp[:, 0].min() >= R.CS_FLOOR, (H, W, sd, comp)
            assert 0.0 < R.finish(comp) < 1.0
    print("%d x %d: smallest CS over sd %s: %.3f" % (H, W, R.SDS, worst))


def test_default_scales_weights_and_finishing():
    for shape, S in (((256, 256), 5), ((64, 64), 3), ((11, 11), 1), ((21, 400), 1), ((22, 22), 2), ((175, 300), 4), ((176, 176), 5),
                     ((4096, 4096), 5)):
        assert MS.default_scales(*shape) == R.default_scales(*shape) == S, shape
    with pytest.raises(ValueError):
        MS.default_scales(10, 64)
    for bad in (0, 6, 4):
        with pytest.raises(ValueError):
            MS.check_scales(64, 64, bad)
    assert MS.check_scales(64, 64, None) == 3 and MS.check_scales(64, 64, 1) == 1
    for S in range(1, 6):
        w = MS.level_weights(S)
        assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w * sum(R.WEIGHTS[:S]), R.WEIGHTS[:S], rtol=1e-15, atol=0)
        assert np.array_equal(w, R.weights(S))
    assert (MS.C1, MS.C2, MS.WEIGHTS) == (R.C1, R.C2, R.WEIGHTS) and R.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert abs(R.C1 - 6.5025) < 1e-14 and abs(R.C2 - 58.5225) < 1e-13
    comp = np.array([[[0.5, 0.4], [0.9, 0.8], [0.7, 0.6]], [[-0.1, 0.4], [0.9, 0.8], [0.7, 0.6]], [[0.5, 0.4], [0.9, 0.8], [0.7, -0.6]]])
    got = MS.finish(comp)
    w = MS.level_weights(3)
    assert abs(got[0] - 0.5 ** w[0] * 0.9 ** w[1] * 0.6 ** w[2]) < 1e-15 and got[1] == 0.0 and got[2] == 0.0
    assert [MS.finish(comp[k:k + 1])[0] for k in range(3)] == [R.finish(comp[k]) for k in range(3)]
    assert np.array_equal(MS.positions(45, 47, 3), [35 * 37, 12 * 13, 1 * 1])
    d = MS.diversity_of(comp[:1].repeat(4, axis=0))
    assert abs(d["mean"] - got[0]) < 1e-15 and d["std"] < 1e-15 and np.allclose(d["per_scale"], comp[0])


def test_random_pairs():
    state = np.random.get_state()[1].copy()
    i, j = MS.random_pairs(7, 1000, 3)
    assert i.shape == j.shape == (1000,) and i.dtype == j.dtype == np.int64
    assert (i != j).all() and i.min() == 0 and i.max() == 6 and j.min() == 0 and j.max() == 6
    assert sorted(set(((j - i) % 7).tolist())) == [1, 2, 3, 4, 5, 6]
    again = MS.random_pairs(7, 1000, 3)
    assert np.array_equal(i, again[0]) and np.array_equal(j, again[1])
    short = MS.random_pairs(7, 10, 3)                                # the first pairs do not depend on how many are drawn
    assert np.array_equal(short[0], i[:10]) and np.array_equal(short[1], j[:10])
    other = MS.random_pairs(7, 1000, 4)
    assert not np.array_equal(i, other[0])
    assert np.array_equal(np.random.get_state()[1], state)           # the global generator is not touched
    two = MS.random_pairs(2, 50, 0)
    assert (two[0] != two[1]).all()
    assert MS.random_pairs(5, 0, 0)[0].shape == (0,)
    for n in (1, 0, -3):
        with pytest.raises(ValueError):
            MS.random_pairs(n, 4, 0)


def test_metric_settings_pickle_and_refusals():
    import torch
    from rna_gan_amd.metrics import PairDiversity
    m = PairDiversity(8, pairs=5, scales=2, seed=9, batch_size=4, encoding_dims=6)
    assert (m.n_fake, m.pairs, m.scales, m.seed, m.batch_size) == (8, 5, 2, 9, 4) and tuple(m.noise.shape) == (8, 6)
    assert PairDiversity(8).pairs == 8
    i, j = m.pair_list()
    assert np.array_equal(i, MS.random_pairs(8, 5, 9)[0]) and np.array_equal(j, MS.random_pairs(8, 5, 9)[1])
    m.history.append({"generated": 0.5, "real": 0.25, "gap": 0.25, "per_scale": [[0.5, 0.4], [0.6, 0.5]]})
    m.set_real(torch.zeros(8, 3, 16, 16, dtype=torch.uint8))
    blob = pickle.dumps(m)
    assert len(blob) < 4096
    back = pickle.loads(blob)
    assert (back.n_fake, back.pairs, back.scales, back.seed, back.batch_size) == (8, 5, 2, 9, 4)
    assert back.history == m.history and back.noise is None and back.real is None and back.last is None and back._real_score is None
    assert set(m.__getstate__()) == {"arg_map", "n_fake", "seed", "batch_size", "pairs", "scales", "history"}
    assert not hasattr(m, "set_train")                              # the CLI hands the resident set to whatever has one
    for bad in (dict(samples=1), dict(samples=0), dict(samples=4, pairs=0), dict(samples=4, scales=6), dict(samples=4, batch_size=0),
                dict(samples=4, real=torch.zeros(3, 3, 16, 16, dtype=torch.uint8)), dict(samples=4, real=torch.zeros(4, 3, 16, 16)),
                dict(samples=4, real=torch.zeros(4, 16, 16, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            PairDiversity(**bad)


def test_cli_parsing(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json", "--loss_type", "wgan"]
    args = H.parse_args(base)
    assert args.div_samples == 0 and args.div_pairs == 0            # off by default
    args = H.parse_args(base + ["--div_samples", "64", "--div_pairs", "100"])
    assert (args.div_samples, args.div_pairs) == (64, 100)
    for bad in (["--div_samples", "1"], ["--div_samples", "-4"], ["--div_samples", "8", "--div_pairs", "-1"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()


def test_wrapper_refuses_on_the_host():
    import torch
    t = torch.zeros(4, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        MS.components(t, None, ([0], [1]))                          # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError):
        MS.components(t.float(), None, ([0], [1]))
    with pytest.raises(ValueError):
        MS.pair_diversity(t, 0)
    assert (MS.BAND, MS.COLS) == (32, 16)
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/rnagan_hip.h").read()
    assert "#define RG_MSSSIM_BAND %d\n" % MS.BAND in header and "#define RG_MSSSIM_COLS %d\n" % MS.COLS in header
