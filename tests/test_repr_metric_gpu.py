"""Per-patient representations and the conditioning metric end to end (rna_gan_amd.representation,
rna_gan_amd.metrics.ConditioningFidelity, Trainer.eval_ops, compute_representation.py).

Planted case: P = 6 patients, each with a pattern of 3 x 4 x 4 values.  A real tile is its patient's pattern plus a little noise.
The stub encoder hands the expression row through (row p = 5 e_p), so after rg_latent_prep's column standardisation column p of
the noise is about sqrt(P - 1) on the rows of patient p and about -1 / sqrt(P - 1) elsewhere; the stub generator reads the patient
back as the argmax over the first P columns and emits that patient's pattern: it honours its conditioning THROUGH the real noise
path.  The stub extractor average-pools the resized image back to 4 x 4: 48 features, the pattern up to the resize's smoothing.
Every generated centroid is then nearest to its own patient's real centroid: all ranks 0 -- checked against the numpy
restatement (tests/repr_refs.py) on the downloaded centroids as well.

The trainer run uses the networks and the resident RNA set of tests/test_resident_trainer_gpu.py's wganvae test: out_size 16,
4 step channels, encoding_dims 2048, fp32, a betaVAE over 64 features with random weights."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from rna_gan_amd import fid as PF
from rna_gan_amd import losses as PL
from rna_gan_amd import representation as RP
from rna_gan_amd.metrics import ConditioningFidelity
from rna_gan_amd.resident import DeviceTileLoader, DeviceTileSet
from repr_refs import group_sums_ref, match_ranks_ref, retrieval_scores_ref
from test_resident_trainer_gpu import _LABELS, _RNA, _ROW_OF, _U8, _network

CUDA = torch.device("cuda:0")
NP, E, S, TPP = 6, 16, 4, 5
_RNG = np.random.default_rng(61)
PATTERNS = torch.from_numpy(_RNG.uniform(-0.8, 0.8, size=(NP, 3, S, S)).astype(np.float32))
ROWS = 5.0 * torch.eye(NP, E)


@pytest.fixture(autouse=True)
def _restore_plugin_globals():
    was = PL.TRAINER_LOOKAHEAD[0], PL._NEXT_NOISE[0]
    yield
    PL.TRAINER_LOOKAHEAD[0], PL._NEXT_NOISE[0] = was


class PassThroughEncoder(nn.Module):
    def encode(self, x):
        return x, None, None


class PatternGenerator(nn.Module):
    """noise (n, E) -> the pattern of argmax(noise[:, :NP]) plus a jitter taken from the noise's other columns"""
    encoding_dims = E

    def __init__(self):
        super().__init__()
        self.patterns = nn.Parameter(PATTERNS.clone(), requires_grad=False)

    def forward(self, noise):
        who = noise[:, :NP].argmax(dim=1)
        return self.patterns[who] + 0.01 * torch.tanh(noise[:, NP:NP + 1]).view(-1, 1, 1, 1)


def pooled(x01):
    return torch.nn.functional.adaptive_avg_pool2d(x01, S).flatten(1)


def _real_set(per_patient=(3, 1, 4, 2, 5, 2)):
    ids = np.concatenate([np.full(k, p) for p, k in enumerate(per_patient)])
    ids = ids[np.random.default_rng(3).permutation(len(ids))]
    tiles = PATTERNS[ids] + 0.02 * torch.from_numpy(np.random.default_rng(4).standard_normal((len(ids), 3, S, S)).astype(np.float32))
    return tiles.to(CUDA), torch.from_numpy(ids.astype(np.int32)).to(CUDA)


def _planted_representations():
    tiles, ids = _real_set()
    G = PatternGenerator().to(CUDA)
    reps = RP.patient_representations(pooled, real=(tiles, ids), conditioned=G, betavae=PassThroughEncoder(), gene_exp=ROWS,
                                      tiles_per_patient=TPP, seed=7, batch_size=7, group=11, resize=299)
    return tiles, ids, G, reps


def test_group_means_and_planted_retrieval():
    tiles, ids, G, reps = _planted_representations()
    real, fake = reps["real"], reps["conditioned"]
    assert sorted(reps) == ["conditioned", "real"] and real.shape == fake.shape == (NP, 3 * S * S)
    assert real.dtype == fake.dtype == torch.float64 and real.is_cuda and fake.is_cuda
    # the real centroids are the sequential fp64 means of the same features, whatever the batching
    feats = pooled(PF.preprocess_images_device(tiles, 299, (-1, 1)))
    sums, counts = group_sums_ref(feats.cpu().numpy(), ids.cpu().numpy(), NP)
    assert np.array_equal(counts, [3, 1, 4, 2, 5, 2])
    assert np.array_equal(real.cpu().numpy().view(np.uint64), (sums / counts[:, None].astype(np.float64)).view(np.uint64))
    acc = RP.GroupMeans(NP, feats.shape[1], CUDA)
    wide = torch.full((feats.shape[0], feats.shape[1] + 3), float("nan"), device=CUDA)
    wide[:, :feats.shape[1]] = feats
    acc.update(wide[:5, :feats.shape[1]], ids[:5]).update(wide[5:, :feats.shape[1]], ids[5:])      # column slices, read in place
    assert torch.equal(acc.means(), real) and acc.counts().tolist() == [3, 1, 4, 2, 5, 2] and acc.n == 17
    with pytest.raises(ValueError, match="no rows"):
        RP.GroupMeans(NP + 1, feats.shape[1], CUDA).update(feats, ids).means()
    with pytest.raises(TypeError):
        acc.update(feats, ids.long())
    with pytest.raises(ValueError):
        acc.update(feats[:, :5], ids)
    # every generated centroid finds its own patient first
    for center in (True, False):
        rank, dtarget = RP.match_ranks(fake, real, center=center)
        assert rank.dtype == torch.int32 and dtarget.dtype == torch.float64 and rank.is_cuda
        assert rank.tolist() == [0] * NP, (center, rank.tolist())
        scores = RP.retrieval_scores(rank, NP)
        assert scores == retrieval_scores_ref(rank.cpu().numpy(), NP)
        assert scores["top1"] == 1.0 and scores["top5"] == 1.0 and scores["mrr"] == 1.0 and scores["median_rank"] == 0.0
        assert scores["chance_top1"] == 1.0 / NP
    a, b = fake.cpu().numpy(), real.cpu().numpy()
    assert match_ranks_ref(a, b)[0].tolist() == [0] * NP, "the planted centroids, checked with the restatement"
    assert match_ranks_ref(a - a.mean(axis=0, keepdims=True), b - b.mean(axis=0, keepdims=True))[0].tolist() == [0] * NP
    # the targets rotated by one: nobody's designated partner is the nearest row
    rotated = (np.arange(NP) + 1) % NP
    rank, _ = RP.match_ranks(fake, real, target=rotated)
    assert (rank > 0).all() and RP.retrieval_scores(rank, NP)["top1"] == 0.0
    assert rank.tolist() == match_ranks_ref(a - a.mean(axis=0, keepdims=True), b - b.mean(axis=0, keepdims=True), rotated)[0].tolist()
    with pytest.raises(ValueError):
        RP.match_ranks(fake, real, target=[0, 1, 2, 3, 4, NP])
    with pytest.raises(ValueError):
        RP.match_ranks(torch.cat([fake, fake]), real)
    with pytest.raises(TypeError):
        RP.match_ranks(fake.float(), real)


def test_a_common_offset_decides_the_ranks_unless_the_sets_are_centred():
    _, _, _, reps = _planted_representations()
    real, fake = reps["real"], reps["conditioned"]
    offset = torch.from_numpy(np.random.default_rng(9).standard_normal(real.shape[1])).to(CUDA) * 50.0
    shifted = fake + offset
    plain = RP.retrieval_scores(RP.match_ranks(shifted, real, center=False)[0], NP)
    centred = RP.retrieval_scores(RP.match_ranks(shifted, real, center=True)[0], NP)
    print("offset of norm %.0f: center=False %r, center=True %r" % (float(offset.norm()), plain, centred))
    assert centred["top1"] == 1.0 and centred["median_rank"] == 0.0
    assert plain["top1"] <= 2.0 / NP and plain["mrr"] < centred["mrr"], "every query ranks the real rows along the offset first"
    h = shifted.cpu().numpy()
    assert RP.match_ranks(shifted, real, center=False)[0].tolist() == match_ranks_ref(h, real.cpu().numpy())[0].tolist()


def test_metric_on_the_planted_case_and_unconditioned_source():
    tiles, ids, G, reps = _planted_representations()
    D = nn.Linear(1, 1).to(CUDA)                               # a fixed extractor never calls the discriminator
    metric = ConditioningFidelity(tiles, ids, ROWS, PassThroughEncoder(), tiles_per_patient=TPP, extractor=pooled, seed=7,
                                  batch_size=7, group=11, report="mrr")
    G.train(); D.train()
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    v = metric.metric_ops(G, D, CUDA)
    assert v == 1.0 and metric.last["top1"] == 1.0 and metric.last_rank.tolist() == [0] * NP and metric.history == [metric.last]
    assert G.training and D.training
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    cached = metric._real_centroids
    assert torch.equal(cached, reps["real"])
    assert metric.metric_ops(G, D, CUDA) == v and metric._real_centroids is cached and len(metric.history) == 2
    for bad in (dict(rna=ROWS[:1]), dict(patient_of=torch.zeros(len(ids), dtype=torch.int32)), dict(patient_of=ids[:-1])):
        kw = dict(real_tiles=tiles, patient_of=ids, rna=ROWS, betavae=PassThroughEncoder())
        kw.update(bad)
        with pytest.raises(ValueError):
            ConditioningFidelity(**kw)
    with pytest.raises(ValueError):
        ConditioningFidelity(tiles, ids, ROWS, PassThroughEncoder(), report="top3")
    # an unconditioned source: its centroids carry no patient, the rows are dealt tile-major
    class Flat(nn.Module):
        encoding_dims = E

        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.zeros(1), requires_grad=False)

        def forward(self, z):
            return torch.tanh(z[:, :1]).view(-1, 1, 1, 1).expand(-1, 3, S, S).contiguous()
    un = RP.patient_representations(pooled, unconditioned=Flat().to(CUDA), n_patients=NP, tiles_per_patient=TPP, seed=2,
                                    batch_size=4, resize=299)["unconditioned"]
    z = torch.randn(NP * TPP, E, generator=torch.Generator().manual_seed(2))
    want = (torch.tanh(z[:, 0]).view(TPP, NP).double() * 0.5 + 0.5)
    # the features are fp32 values in [0, 1]: the stub extractor's pooling adds 75 x 75 = 5625 of them per cell in fp32, in an order
    # of torch's choosing -- at most 5625 u_fp32 relative, u_fp32 = 2^-24, on values <= 1 -- and the tanh, the taps and the division
    # add a few ulp: 5700 * 2^-24 = 3.4e-4.  A row dealt to another patient moves a mean by 0.01 and more.
    print("unconditioned centroids: max |device - host| = %.3g" % float((un[:, 0].cpu() - want.mean(dim=0)).abs().max()))
    assert un.shape == (NP, 3 * S * S) and torch.allclose(un[:, 0].cpu(), want.mean(dim=0), rtol=0, atol=5700 * 2.0 ** -24)


# ------------------------------------------------------------------ the Trainer
def _tileset():
    return DeviceTileSet.from_tensors(torch.from_numpy(_U8.copy()), rna=torch.from_numpy(_RNA.copy()),
                                      row_of=torch.from_numpy(_ROW_OF.copy()), labels=torch.from_numpy(_LABELS.copy()), device=CUDA)


def _run(tmp_path, tag, with_metric, epochs=2):
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    ts = _tileset()
    loader = DeviceTileLoader(ts, 6, transform=None, seed=8, rank=0)
    kw = dict(checkpoint=None, rna_features=_RNA.shape[1])
    losses = [P.WassersteinGeneratorLossVAE(**kw), P.WassersteinDiscriminatorLossVAE(**kw), P.WassersteinGradientPenaltyVAE(**kw)]
    metrics = None
    if with_metric:
        metrics = [ConditioningFidelity.from_tile_set(ts, losses[0].betavae, tiles_per_patient=3, seed=4, batch_size=8, group=7)]
    tr = P.Trainer(_network(2048), losses, metrics_list=metrics, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4,
                   epochs=epochs, recon=None, precision="fp32")
    tr(loader)
    torch.cuda.synchronize()
    return tr, ts, losses


def _state(m):
    return [t.detach().clone() for t in list(m.parameters()) + list(m.buffers())]


def test_trainer_logs_the_metric_and_trains_the_same_weights(tmp_path):
    tr, ts, losses = _run(tmp_path, "m", True)
    log = tr.metric_logs["ConditioningFidelity"]
    live = tr.metrics["ConditioningFidelity"]
    assert len(log) == 2 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in log)
    assert len(live.history) == 2 and [h["top1"] for h in live.history] == log and live.history[-1] == live.last
    assert sorted(live.last) == ["chance_top1", "median_rank", "mrr", "top1", "top5"] and live.last["chance_top1"] == 0.2
    print("ConditioningFidelity per epoch: %r" % live.history)
    # the last entry is a stand-alone patient_representations + match_ranks call on the trained networks, bit for bit
    G, D = tr.generator, tr.discriminator
    was = G.training, D.training
    G.eval(); D.eval()
    reps = RP.patient_representations(PF.discriminator_features_device(D), real=ts, conditioned=G, betavae=losses[0].betavae,
                                      gene_exp=ts.rna, tiles_per_patient=3, seed=4, batch_size=8, group=7)
    G.train(was[0]); D.train(was[1])
    rank, _ = RP.match_ranks(reps["conditioned"], reps["real"])
    assert reps["real"].shape == (5, reps["conditioned"].shape[1]) and torch.equal(rank, live.last_rank)
    assert RP.retrieval_scores(rank, 5) == live.last
    assert live._real_centroids is None                        # the extractor moves with training: nothing is cached
    # the same run without the metric: the same weights
    off, _, _ = _run(tmp_path, "p", False)
    assert off.metric_logs == {} and off.loss_logs == tr.loss_logs
    for a, b in zip(_state(tr.generator) + _state(tr.discriminator), _state(off.generator) + _state(off.discriminator)):
        assert torch.equal(a, b)
    # a pickle keeps the settings and the history only
    blob = pickle.dumps(live)
    assert len(blob) < 16 * 1024
    back = pickle.loads(blob)
    assert (back.tiles_per_patient, back.seed, back.batch_size, back.group, back.center, back.report, back.extractor) == \
        (3, 4, 8, 7, True, "top1", "discriminator")
    assert back.history == live.history and back.last is None and back.last_rank is None
    assert back.real_tiles is None and back.patient_of is None and back.rna is None and back.betavae is None
    with pytest.raises(RuntimeError, match="set_data"):
        back.metric_ops(G, D, CUDA)
    back.set_data(ts.tiles, ts.row_of, ts.rna, losses[0].betavae)
    assert back.metric_ops(G, D, CUDA) == log[-1] and back.history[-1] == live.last
    ck = torch.load(str(tmp_path / "ganm1.model"), map_location="cpu", weights_only=False)
    assert ck["metric_logs"] == {"ConditioningFidelity": log[:1]}
    assert ck["metric_objects"]["ConditioningFidelity"].history == live.history[:1]


# ------------------------------------------------------------------ compute_representation.py
def test_compute_representation_synthetic(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import json
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"path_csv": ["synthetic"], "patch_data_path": ["synthetic"], "img_size": 32, "rna_features": 16,
                               "max_patch_per_wsi": 4, "synthetic_patients": 5}))
    prefix = str(tmp_path / "rep")
    cmd = [sys.executable, os.path.join(repo, "compute_representation.py"), "--config", str(cfg), "--synthetic", "--sample_size", "4",
           "--seed", "3", "--gan", "random", "--vaegan", "random", "--path_to_save", prefix, "--multiprocessing"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    arrays = {k: np.load(prefix + "_%s.npy" % k) for k in ("real", "vaegan", "gan")}
    F = arrays["real"].shape[1]
    assert all(a.shape == (5, F) and a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert "top1" in r.stdout and "chance_top1" in r.stdout
    import compute_representation as CR
    args = CR.parse_args(cmd[2:])
    out = CR.run(args)
    assert np.array_equal(out["conditioned"].float().cpu().numpy().view(np.uint32), arrays["vaegan"].view(np.uint32))
    assert np.array_equal(out["real"].float().cpu().numpy().view(np.uint32), arrays["real"].view(np.uint32))
    # without --gan no _gan.npy is written
    os.remove(prefix + "_gan.npy")
    CR.run(CR.parse_args(["--config", str(cfg), "--synthetic", "--sample_size", "4", "--seed", "3", "--path_to_save", prefix]))
    assert not os.path.exists(prefix + "_gan.npy")
    assert np.array_equal(np.load(prefix + "_vaegan.npy").view(np.uint32), arrays["vaegan"].view(np.uint32))
