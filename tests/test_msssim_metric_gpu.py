"""The pixel-space diversity end to end (rna_gan_amd.msssim.pair_diversity, rna_gan_amd.metrics.PairDiversity, Trainer.eval_ops,
the CLI's --div_samples) with tiny networks at 64 x 64 (S = 3): what the metric logs EQUALS msssim.ms_ssim on the same generated
bytes, and the numpy restatement of tests/msssim_refs.py within the tolerance of tests/test_msssim_ops_gpu.py."""
import pickle

import numpy as np
import pytest
import torch
from torch import nn
from torch.optim import Adam
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
import msssim_refs as R
from rna_gan_amd import msssim as MS
from rna_gan_amd.metrics import PairDiversity, TissueYield
from rna_gan_amd.resident import DeviceTileSet
from rna_gan_amd.synth import synthetic_images, synthetic_tiles_u8

CUDA = torch.device("cuda:0")
IN_SIZE, STEP, ENC, BATCH = 64, 4, 24, 8
TOL = 1e-9
KEYS = {"generated", "real", "gap", "per_scale"}


@pytest.fixture(autouse=True)
def _leave_the_loss_plugins_as_found():
    """as tests/test_tissue_metric_gpu.py: a Trainer switches the plugins' process-wide look-ahead on; put it back"""
    from rna_gan_amd import losses as L
    flag, pending = L.TRAINER_LOOKAHEAD[0], L._NEXT_NOISE[0]
    yield
    L.TRAINER_LOOKAHEAD[0], L._NEXT_NOISE[0] = flag, pending


def network():
    return {
        "generator": {"name": P.DCGANGenerator,
                      "args": {"encoding_dims": ENC, "out_channels": 3, "step_channels": STEP, "out_size": IN_SIZE,
                               "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.Tanh()},
                      "optimizer": {"name": Adam, "args": {"lr": 0.0001, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": {"in_size": IN_SIZE, "in_channels": 3, "step_channels": STEP,
                                   "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.LeakyReLU(0.2)},
                          "optimizer": {"name": Adam, "args": {"lr": 0.0004, "betas": (0.5, 0.999)}}},
    }


def _generator(seed):
    torch.manual_seed(seed)
    net = network()["generator"]
    return net["name"](**net["args"]).cuda()


def test_pair_diversity_of_copies_and_of_distinct_tiles():
    a, _ = R.correlated_sets(16, 64, 64, 16, seed=9)
    one = torch.from_numpy(a[:1].repeat(16, axis=0)).to(CUDA)
    d = MS.pair_diversity(one, 12, seed=3)
    assert d["mean"] == 1.0 and d["std"] == 0.0 and np.array_equal(d["per_scale"], np.ones((3, 2)))
    # 16 distinct correlated tiles: tile k is the base tile plus N(0, 8 + 4 k) noise
    base = a[0].astype(np.float64)
    rng = np.random.default_rng(12)
    tiles = np.stack([np.clip(np.rint(base + rng.normal(0.0, 8.0 + 4.0 * k, size=base.shape)), 0, 255).astype(np.uint8) for k in range(16)])
    pairs = MS.random_pairs(16, 8, seed=3)
    want = R.batch_components(tiles, tiles, pairs)
    wscore = np.array([R.finish(c) for c in want])
    assert want[:, :, 0].min() >= R.CS_FLOOR
    for layout, t in (("nhwc", tiles), ("nchw", tiles.transpose(0, 3, 1, 2))):
        dev = torch.from_numpy(np.ascontiguousarray(t)).to(CUDA)
        got = MS.pair_diversity(dev, 8, seed=3, layout=layout)
        assert abs(got["mean"] - wscore.mean()) <= TOL and abs(got["std"] - wscore.std()) <= TOL
        assert np.abs(np.array(got["per_scale"]) - want.mean(axis=0)).max() <= TOL
        assert np.abs(MS.ms_ssim(dev, None, pairs, layout=layout) - wscore).max() <= TOL
    print("pair_diversity of 16 correlated tiles: %r" % got)
    ts = DeviceTileSet.from_tensors(torch.from_numpy(np.ascontiguousarray(tiles.transpose(0, 3, 1, 2))), device=CUDA)
    assert MS.pair_diversity(ts, 8, seed=3) == got
    # two sets row by row, plain SSIM, and the host's index check
    dev = torch.from_numpy(tiles).to(CUDA)
    s1 = MS.ssim(dev[:4], dev[4:8])
    assert np.abs(s1 - np.array([R.ms_ssim(tiles[k], tiles[4 + k], 1) for k in range(4)])).max() <= TOL
    assert MS.components(dev, None, ([], [])).shape == (0, 3, 2)
    for bad in (([0], [16]), ([-1], [0]), ([0, 1], [1]), ([0.5], [1.0])):
        with pytest.raises(ValueError):
            MS.components(dev, None, bad)
    with pytest.raises(ValueError):
        MS.components(dev, None, None)                              # pairs=None needs two sets
    with pytest.raises(ValueError):
        MS.components(dev, dev[:3])
    with pytest.raises(ValueError):
        MS.components(dev, None, ([0], [1]), scales=4)


def test_metric_equals_ms_ssim_on_its_own_tiles_caches_real_and_pickles():
    G = _generator(3)
    real = synthetic_tiles_u8(12, IN_SIZE, 5).to(CUDA)              # (N, 3, H, W)
    metric = PairDiversity(12, pairs=7, real=real, batch_size=5, seed=4)        # 5 + 5 + 2: a ragged last batch
    G.train()
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    v1 = metric.metric_ops(G, CUDA)
    first = dict(metric.last)
    tiles = torch.cat(metric.generated_tiles(G, CUDA))
    assert tiles.dtype == torch.uint8 and tuple(tiles.shape) == (12, IN_SIZE, IN_SIZE, 3)
    pairs = metric.pair_list()
    scores = MS.ms_ssim(tiles, None, pairs)
    assert np.array_equal(metric.last_scores, scores) and v1 == first["generated"] == float(scores.mean())
    # against the restatement: the components (a CS of a random generator's tiles may sit near the clamp, where the power is
    # ill-conditioned), and the device's own finishing of them
    comp = MS.components(tiles, None, pairs)
    host = tiles.cpu().numpy()
    assert np.abs(comp - R.batch_components(host, host, pairs)).max() <= TOL and np.array_equal(MS.finish(comp), scores)
    assert np.array_equal(first["per_scale"], comp.mean(axis=0)) and comp.shape == (7, 3, 2)
    real_scores = MS.ms_ssim(real, None, pairs, layout="nchw")
    assert set(first) == KEYS and first["real"] == float(real_scores.mean()) and first["gap"] == first["generated"] - first["real"]
    cached = metric._real_score
    metric.real = None                                               # the second evaluation must not look at the real tiles again
    v2 = metric.metric_ops(G, CUDA)
    assert v2 == v1 and metric._real_score == cached and metric.history == [first, first]
    assert G.training and torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), dev_rng)
    blob = pickle.dumps(metric)
    assert len(blob) < 16 * 1024
    back = pickle.loads(blob)
    assert back.history == metric.history and back.noise is None and back.real is None and back._real_score is None
    assert back.metric_ops(G, CUDA) == v1 and back.last["real"] is None and back.last["gap"] is None
    back.set_real(DeviceTileSet.from_tensors(real.cpu(), device=CUDA))
    assert back.metric_ops(G, CUDA) == v1 and back.last == first


def test_a_generator_that_ignores_its_noise_scores_one():
    G = _generator(6)
    with torch.no_grad():
        hit = [p for p in G.parameters() if ENC in p.shape]
        assert len(hit) == 1, "the first layer is the one parameter with an encoding_dims axis"
        hit[0].zero_()
    real = synthetic_tiles_u8(8, IN_SIZE, 7).to(CUDA)
    metric = PairDiversity(8, real=real, batch_size=8, seed=1)
    assert metric.metric_ops(G, CUDA) == 1.0
    tiles = torch.cat(metric.generated_tiles(G, CUDA))
    assert bool((tiles == tiles[:1]).all()), "zeroed first-layer weights: every tile is the same tile"
    assert metric.last["generated"] == 1.0 and metric.last["gap"] == 1.0 - metric.last["real"] and 0.0 <= metric.last["real"] < 0.5
    assert np.array_equal(metric.last["per_scale"], np.ones((3, 2)))


def _loader():
    imgs = synthetic_images(2 * BATCH, IN_SIZE, seed=5)
    return DataLoader(TensorDataset(imgs, torch.zeros(2 * BATCH)), batch_size=BATCH)


def _trainer(tmp_path, tag, metrics, epochs=2):
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    return P.Trainer(network(), losses, metrics_list=metrics, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4, epochs=epochs,
                     recon=str(tmp_path / ("img" + tag)), nrow=2)


def test_trainer_logs_the_diversity_and_the_history_survives_a_checkpoint(tmp_path):
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    real = synthetic_tiles_u8(BATCH, IN_SIZE, 9).to(CUDA)
    tr = _trainer(tmp_path, "m", [PairDiversity(BATCH, real=real, batch_size=BATCH, seed=8), TissueYield(BATCH, batch_size=BATCH, seed=8)])
    tr(_loader())
    torch.cuda.synchronize()
    live = tr.metrics["PairDiversity"]
    log = tr.metric_logs["PairDiversity"]
    assert sorted(tr.metric_logs) == ["PairDiversity", "TissueYield"] and len(log) == 2
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in log) and [h["generated"] for h in live.history] == log
    assert all(set(h) == KEYS for h in live.history) and live.history[0]["real"] == live.history[1]["real"]
    print("PairDiversity per epoch: %r" % live.history)
    tiles = torch.cat(live.generated_tiles(tr.generator, CUDA))     # the evaluation of the last epoch ran on this generator
    assert log[-1] == float(MS.ms_ssim(tiles, None, live.pair_list()).mean())
    path = str(tmp_path / "ganm1.model")                            # written before epoch 2's evaluation: it holds epoch 1's values
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["metric_logs"]["PairDiversity"] == log[:1]
    saved = ck["metric_objects"]["PairDiversity"]
    assert saved.history == live.history[:1] and saved.noise is None and saved.real is None and (saved.n_fake, saved.pairs, saved.seed) == (BATCH, BATCH, 8)
    again = _trainer(tmp_path, "b", [PairDiversity(BATCH, real=real, batch_size=BATCH, seed=8), TissueYield(BATCH, batch_size=BATCH, seed=8)],
                     epochs=3)
    again.load_model(load_path=path)
    assert again.metrics["PairDiversity"].history == live.history[:1] and again.metric_logs["PairDiversity"] == log[:1]
    again(_loader())
    assert len(again.metric_logs["PairDiversity"]) == 2 and len(again.metrics["PairDiversity"].history) == 2


def test_through_the_cli(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json", "--loss_type", "wgan", "--seed", "5", "--synthetic"]
    with pytest.raises(SystemExit):
        H.parse_args(base + ["--div_samples", "1"])
    capsys.readouterr()
    args = H.parse_args(base + ["--div_samples", "8", "--qc_samples", "8"])
    assert args.synthetic and args.div_samples == 8 and args.div_pairs == 0
    ds = H.SyntheticTiles(8, IN_SIZE, 4, False, 0)
    holder = {}
    qc = H.build_qc_metric(args, ds, [], CUDA, holder)
    div = H.build_div_metric(args, ds, [], CUDA, holder)
    assert isinstance(div, PairDiversity) and (div.n_fake, div.pairs, div.seed, div.batch_size) == (8, 8, 5, 8) and div.noise is qc.noise
    # the real baseline is the first 8 items turned back to the bytes they came from
    items = torch.stack([ds[k][0] for k in range(8)])
    assert div.real.dtype == torch.uint8 and tuple(div.real.shape) == (8, IN_SIZE, IN_SIZE, 3)
    assert torch.equal(div.real.cpu(), torch.round((items * 0.5 + 0.5) * 255.0).to(torch.uint8).permute(0, 2, 3, 1))
    G = _generator(6)
    v = div.metric_ops(G, CUDA)
    tiles = torch.cat(div.generated_tiles(G, CUDA))
    assert v == float(MS.ms_ssim(tiles, None, div.pair_list()).mean())
    assert div.last["real"] == float(MS.ms_ssim(div.real, None, div.pair_list()).mean()) and div.last["gap"] == v - div.last["real"]
    few = H.build_div_metric(H.parse_args(base + ["--div_samples", "8", "--div_pairs", "3"]), ds, [], CUDA, {})
    assert few.pairs == 3
