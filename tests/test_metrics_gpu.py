"""The device-side Frechet-distance evaluation end to end (rna_gan_amd.fid device path, rna_gan_amd.metrics.FrechetDistance,
Trainer.eval_ops) with tiny networks: in_size 32, step_channels 4 (F = 16 trunk features), encoding_dims 16, batch 8.

Counted bound of the statistics.  The device and the host path see the same fp32 features X (n rows); they differ in how
fp64 sums are ordered and in the covariance formula (raw moments against np.cov's centred product).  With u = 2^-53,
d = diag(X^T X) and D = sqrt(d d^T) -- which bounds |s2|, |X|^T |X| and n |mu mu^T| elementwise (Cauchy-Schwarz):
  device: s2 carries n u D (tests/test_fid_device_ops_gpu.py), n mu mu^T (2 n + 3) u D from the error of s1, the subtraction
          and the division 4 u D more: (3 n + 8) u D / (n - 1);
  host:   np.cov's centred product n u D, the error of its mean entering twice with n u D each, a few roundings: (3 n + 4) u D / (n - 1);
together (6 n + 12) u D / (n - 1) <= 8 n u D / (n - 1) for n >= 6, the smallest set used here.  For the mean: both sides sum
n terms, (2 n + 2) u mean|x| <= 4 n u mean|x|.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import Adam
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from oracle import ref_cpu as R
from rna_gan_amd import fid as PF
from rna_gan_amd.metrics import FrechetDistance
from rna_gan_amd.synth import synthetic_tiles_u8

IN_SIZE, STEP, ENC, BATCH = 32, 4, 16, 8
U = 2.0 ** -53


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


def _models(seed=0):
    torch.manual_seed(seed)
    net = network()
    G = net["generator"]["name"](**net["generator"]["args"]).cuda()
    D = net["discriminator"]["name"](**net["discriminator"]["args"]).cuda()
    with torch.no_grad():                                   # running statistics that are not the initial (0, 1)
        g = torch.Generator().manual_seed(seed + 1)
        for m in (G, D):
            for name, b in m.named_buffers():
                if name.endswith("running_mean"):
                    b.copy_(0.1 * torch.randn(b.shape, generator=g))
                elif name.endswith("running_var"):
                    b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return G, D


def _assert_statistics_close(dev, host, feats, what):
    """(mu, sigma) of the device path against the host path's, within the counted bound of the module docstring"""
    x = np.asarray(feats, dtype=np.float64)
    n = x.shape[0]
    assert n >= 6
    d = (x * x).sum(axis=0)
    m2 = np.sqrt(np.outer(d, d))
    e_mu = float(np.abs(dev[0] - host[0]).max())
    e_sig = np.abs(dev[1] - host[1])
    b_sig = 8 * n * U * m2 / (n - 1)
    b_mu = 4 * n * U * np.abs(x).mean(axis=0)
    print("%s: max |mu diff| %.3g, max |sigma diff| %.3g (bound at that entry %.3g)" % (
        what, e_mu, float(e_sig.max()), float(b_sig.flat[int(e_sig.argmax())])))
    assert np.all(np.abs(dev[0] - host[0]) <= b_mu), what
    assert np.all(e_sig <= b_sig), what
    assert np.array_equal(dev[1], dev[1].T), what


def test_device_statistics_match_the_host_path():
    G, D = _models()
    images = R.synthetic_images(64, IN_SIZE, seed=9)
    host_feats = PF.discriminator_features(D, images, batch_size=BATCH)
    assert host_feats.shape == (64, 16)
    host = PF.activation_statistics(host_feats)
    dev_images = images.cuda()
    extract = PF.discriminator_features_device(D)
    seen = []

    def spy(batch):
        f = extract(batch)
        seen.append(f.cpu().numpy())
        return f
    D.train()
    mu, sigma, n = PF.device_statistics((dev_images[i:i + BATCH] for i in range(0, 64, BATCH)), spy)
    assert n == 64 and D.training
    assert np.array_equal(np.concatenate(seen).view(np.uint32), host_feats.view(np.uint32)), "the features must be bit-identical"
    _assert_statistics_close((mu, sigma), host, host_feats, "discriminator features, 64 images")


# ------------------------------------------------------------------ Inception extractor (seeded random weights)
def _seeded_inception_state(seed):
    """the seeded random-weight network of tests/test_inception_gpu.py (rebuilt here)"""
    from oracle.inception_ref import OracleInception3
    torch.manual_seed(seed)
    o = OracleInception3().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(o.named_parameters()) + list(o.named_buffers()):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            elif name.endswith("bn.weight"):
                t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g))
            elif name.endswith("bias"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            else:
                fan_in = int(np.prod(t.shape[1:]))
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5)
    return o.state_dict()


@pytest.fixture(scope="module")
def inception():
    """the device-side extractor, remembering the features of a batch it has seen (the same batches recur below: the network
    runs once per distinct batch)"""
    extract = PF.inception_features_device(_seeded_inception_state(12))
    seen = {}

    def cached(x01):
        key = hash(x01.cpu().numpy().tobytes())
        if key not in seen:
            seen[key] = extract(x01)
        return seen[key]
    return cached


def test_calculate_fid_on_device(inception):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(6, 64, 64, 3), dtype=np.uint8)
    b = rng.integers(0, 200, size=(6, 64, 64, 3), dtype=np.uint8)
    stats = {}
    for name, imgs in (("a", a), ("b", b)):
        mu, sigma, n = PF.fid_statistics_device(imgs, inception, batch_size=3)
        assert n == 6 and mu.shape == (2048,) and sigma.shape == (2048, 2048)
        # the same statistics composed by hand: device resize -> features -> numpy float64
        t = torch.from_numpy(imgs).cuda()
        x = PF.preprocess_images_device(t, 299)
        assert x.shape == (6, 3, 299, 299) and x.dtype == torch.float32 and x.is_cuda
        feats = torch.cat([inception(x[i:i + 3]) for i in (0, 3)]).cpu().numpy()
        _assert_statistics_close((mu, sigma), PF.activation_statistics(feats), feats, "inception features, set " + name)
        stats[name] = (mu, sigma)
    d_ab = PF.calculate_fid(a, b, inception, batch_size=3, on_device=True)
    d_aa = PF.calculate_fid(a, a, inception, batch_size=3, on_device=True)
    assert d_ab == PF.frechet_distance(*stats["a"], *stats["b"])                       # the distance adds no device arithmetic
    assert np.isfinite(d_ab) and d_ab > 0
    assert abs(d_aa) < 1e-3 * max(1.0, abs(d_ab))


def test_preprocess_images_device_forms():
    rng = np.random.default_rng(4)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(2, 40, 24, 3), dtype=np.uint8)).cuda()
    y = PF.preprocess_images_device(u8, 299)
    host = PF.preprocess_images(u8.cpu().numpy())
    assert float((y.cpu() - host).abs().max()) <= 4 * float(np.spacing(np.nextafter(np.float32(40), np.float32(0)))) + 8 * 2.0 ** -24
    assert torch.equal(PF.preprocess_images_device(u8.permute(0, 3, 1, 2), 299), y)                    # NCHW view: strides only
    f01 = (u8.cpu().float() / 255).cuda()                    # the host transform's division (IEEE), as the kernel's uint8 tap
    assert torch.equal(PF.preprocess_images_device(f01, 299, value_range=(0, 1)), y)
    pm1 = ((u8.cpu().float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous().cuda()
    z = PF.preprocess_images_device(pm1, 299, value_range=(-1, 1))
    assert float((z - y).abs().max()) <= 2.0 ** -23                                                    # the taps differ by an ulp
    assert PF.preprocess_images_device(pm1, 24, value_range=(-1, 1)).shape == (2, 3, 24, 24)
    with pytest.raises(ValueError):
        PF.preprocess_images_device(f01, 299)                                                          # the range is never guessed
    with pytest.raises(ValueError):
        PF.preprocess_images_device(f01, 299, value_range=(0, 255))
    with pytest.raises(ValueError):
        PF.preprocess_images_device(torch.zeros(2, 3, 5, 3, dtype=torch.uint8, device="cuda"))         # which axis is the channel?
    assert PF.preprocess_images_device(torch.zeros(2, 3, 5, 3, dtype=torch.uint8, device="cuda"), 7, layout="NCHW").shape == (2, 3, 7, 7)
    with pytest.raises(TypeError):
        PF.preprocess_images_device(u8.double(), 299, value_range=(0, 1))


def test_feature_moments_object():
    m = PF.FeatureMoments(16, "cuda:0")
    with pytest.raises(ValueError):
        m.statistics()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(40, 24, generator=g).cuda()
    m.update(x[:8, :16]).update(x[8:9, :16]).update(x[9:, :16].contiguous())      # rows of stride 24, one row, packed rows
    assert m.n == 40
    with pytest.raises(ValueError):
        m.update(x[:, :15])
    with pytest.raises(TypeError):
        m.update(x[:, :16].cpu())
    feats = x[:, :16].cpu().numpy()
    _assert_statistics_close(m.statistics(), PF.activation_statistics(feats), feats, "FeatureMoments, 40 x 16")


# ------------------------------------------------------------------ the metric
def _state(m):
    return [t.detach().clone() for t in list(m.parameters()) + list(m.buffers())]


def test_metric_ops_is_repeatable_and_leaves_the_networks_alone():
    G, D = _models(3)
    real = R.synthetic_images(32, IN_SIZE, seed=11).cuda()
    metric = FrechetDistance(real, n_fake=32, batch_size=BATCH, seed=4)
    G.train(); D.train()
    before = _state(G) + _state(D)
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    v1 = metric.metric_ops(G, D, torch.device("cuda:0"))
    v2 = metric.metric_ops(G, D, torch.device("cuda:0"))
    assert isinstance(v1, float) and np.isfinite(v1) and v1 == v2
    assert G.training and D.training
    assert all(torch.equal(a, b) for a, b in zip(before, _state(G) + _state(D))), "running statistics / parameters moved"
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    G.eval()
    assert metric.metric_ops(G, D, torch.device("cuda:0")) == v1 and not G.training and D.training
    # the proxy by hand: eval-mode generator on the metric's noise, host statistics
    with torch.no_grad():
        fake = torch.cat([G(z.cuda()) for z in torch.split(metric.noise, BATCH)])
    want = PF.fid_proxy(D, fake.cpu(), real.cpu(), batch_size=BATCH)
    assert abs(v1 - want) <= 1e-5 * max(1.0, abs(want)), (v1, want)
    # uint8 real tiles give the value of their normalised form
    u8 = synthetic_tiles_u8(32, IN_SIZE, seed=11)
    norm = (u8.float() / 255.0 - 0.5) / 0.5
    a = FrechetDistance(u8.cuda(), batch_size=BATCH, seed=4).metric_ops(G, D, torch.device("cuda:0"))
    b = FrechetDistance(norm.cuda(), batch_size=BATCH, seed=4).metric_ops(G, D, torch.device("cuda:0"))
    assert a == b


class _RealAsFake(nn.Module):
    """a 'generator' that returns the real set: the fake source swapped for the real one"""
    encoding_dims = 1

    def __init__(self, real):
        super().__init__()
        self.real, self.pos = real, 0

    def forward(self, z):
        out = self.real[self.pos:self.pos + z.shape[0]]
        self.pos = (self.pos + z.shape[0]) % self.real.shape[0]
        return out


def test_metric_of_the_real_set_against_itself_is_zero(inception):
    G, D = _models(5)
    real = R.synthetic_images(32, IN_SIZE, seed=12).cuda()
    other = FrechetDistance(real, batch_size=BATCH, seed=1).metric_ops(G, D, torch.device("cuda:0"))
    same = FrechetDistance(real, batch_size=BATCH, seed=1).metric_ops(_RealAsFake(real), D, torch.device("cuda:0"))
    print("discriminator proxy: d(real, real) %.3g, d(fake, real) %.3g" % (same, other))
    assert abs(same) < 1e-3 * max(1.0, abs(other))
    # a callable extractor: resized to 299, real statistics cached after the first call
    real6 = real[:6]
    m = FrechetDistance(real6, extractor=inception, batch_size=3, seed=1)
    same = m.metric_ops(_RealAsFake(real6), D, torch.device("cuda:0"))
    assert m._real_stats is not None and m._real_stats[2] == 6
    print("inception extractor: d(real, real) %.3g" % same)
    assert abs(same) < 1e-3                                  # the margin at its floor, max(1, d) = 1


# ------------------------------------------------------------------ the Trainer
def _loader():
    imgs = R.synthetic_images(2 * BATCH, IN_SIZE, seed=5)
    return DataLoader(TensorDataset(imgs, torch.zeros(2 * BATCH)), batch_size=BATCH)


def _trainer(tmp_path, tag, metrics):
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    return P.Trainer(network(), losses, metrics_list=metrics, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4, epochs=2,
                     recon=str(tmp_path / ("img" + tag)), nrow=2)


def _metric():
    return FrechetDistance(R.synthetic_images(16, IN_SIZE, seed=21).cuda(), batch_size=BATCH, seed=8)


def test_observer_changes_nothing(tmp_path):
    """Two trainer runs from the same seeds, 2 epochs x 2 iterations, with and without the metric: losses, parameters, buffers
    and Adam moments identical bit for bit; the log has one entry per epoch in the first run and does not exist in the second."""
    res = {}
    for with_metric in (True, False):
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        tr = _trainer(tmp_path, "m" if with_metric else "p", [_metric()] if with_metric else None)
        tr(_loader())
        torch.cuda.synchronize()
        og, od = tr.optimizer_generator, tr.optimizer_discriminator
        res[with_metric] = (tr.loss_logs, _state(tr.generator) + _state(tr.discriminator),
                            [og._m.clone(), og._v.clone(), od._m.clone(), od._v.clone(), og._step_dev.clone()], tr.metric_logs,
                            tr.generator.training, tr.discriminator.training)
    on, off = res[True], res[False]
    assert on[0] == off[0] and all(len(v) == 4 for v in on[0].values())
    for k in (1, 2):
        assert len(on[k]) == len(off[k])
        for a, b in zip(on[k], off[k]):
            assert torch.equal(a, b)
    assert list(on[3]) == ["FrechetDistance"] and len(on[3]["FrechetDistance"]) == 2 and off[3] == {}
    assert all(isinstance(v, float) and np.isfinite(v) for v in on[3]["FrechetDistance"])
    assert on[4:] == off[4:]


def test_checkpoint_with_the_metric_loads_with_and_without_it(tmp_path):
    torch.manual_seed(0)
    tr = _trainer(tmp_path, "a", [_metric()])
    tr(_loader())
    assert len(tr.metric_logs["FrechetDistance"]) == 2
    # an epoch's checkpoint is written before its evaluation (torchgan's order): the file of epoch 2 holds epoch 1's value
    log = tr.metric_logs["FrechetDistance"][:1]
    path = str(tmp_path / "gana1.model")
    with_metric = _trainer(tmp_path, "b", [_metric()])
    with_metric.load_model(load_path=path)
    assert with_metric.metric_logs == {"FrechetDistance": log} and with_metric.start_epoch == 2
    without = _trainer(tmp_path, "c", None)
    without.load_model(load_path=path)
    assert without.metric_logs == {"FrechetDistance": log} and without.metrics == {}
    for a, b in zip(tr.generator.state_dict().values(), without.generator.state_dict().values()):
        assert torch.equal(a.cpu(), b.cpu())
    # the loaded trainer with the metric goes on evaluating
    with_metric.epochs = 3
    with_metric(_loader())
    assert len(with_metric.metric_logs["FrechetDistance"]) == 2 and with_metric.metric_logs["FrechetDistance"][0] == log[0]
