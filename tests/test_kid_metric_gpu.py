"""The kernel distance end to end (rna_gan_amd.kid, rna_gan_amd.metrics.KernelDistance, Trainer.eval_ops) with the tiny networks
of tests/test_metrics_gpu.py: in_size 32, step_channels 4 (F = 16 trunk features), encoding_dims 16, batch 8.

Counted bound of the estimate.  Device and host see the same fp32 features and form the same kernel values bit for bit
(tests/test_kid_ops_gpu.py); they differ in the order of the sums.  With u = 2^-53 and A_xx = sum |k(x_i, x_j)| etc.:
  a tile's sum, <= 4096 terms in the kernel's order against the exact sum: 4096 u A_tile (tests/test_kid_ops_gpu.py); over the
  tiles: 4096 u A;  the two fsum roundings (the product adds the tile sums, the restatement all values): 2 u A;
  the diagonal sums, <= 64 terms per tile, 66 u A_diag with A_diag <= A;
  the estimator's own arithmetic, <= 4 roundings per term on either side: 8 u per term;
so every one of the three terms S / (count) carries at most (4096 + 2 + 66 + 8) u <= 4200 u times A / count:
  |mmd2_dev - mmd2_ref| <= 4200 u (A_xx / (m (m - 1)) + A_yy / (n (n - 1)) + 2 A_xy / (m n))."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from oracle import ref_cpu as R
from rna_gan_amd import fid as PF
from rna_gan_amd import kid as KID
from rna_gan_amd.metrics import FrechetDistance, KernelDistance
from kid_refs import U, mmd2_abs_scale, mmd2_unbiased_ref
from test_metrics_gpu import BATCH, IN_SIZE, _models, _state, network

CUDA = torch.device("cuda:0")


def _bound(x, y, **kw):
    m, n = len(x), len(y)
    axx, ayy, axy = mmd2_abs_scale(x, y, **kw)
    return 4200 * U * (axx / (m * (m - 1.0)) + ayy / (n * (n - 1.0)) + 2.0 * axy / (m * float(n)))


def _assert_estimate(got, x, y, what, **kw):
    want, bound = mmd2_unbiased_ref(x, y, **kw), _bound(x, y, **kw)
    print("%s: device %.17g, restatement %.17g, |diff| %.3g (bound %.3g)" % (what, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound, what


@pytest.fixture(scope="module")
def feature_sets():
    """device features of 48 generated and 64 real images through the discriminator trunk, and their host copies"""
    G, D = _models(2)
    extract = PF.discriminator_features_device(D)
    real = R.synthetic_images(64, IN_SIZE, seed=9).cuda()
    z = torch.randn(48, 16, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        G.eval()
        fake = [G(c) for c in torch.split(z, BATCH)]
    x = PF.device_features(fake, extract)
    y = PF.device_features((real[i:i + BATCH] for i in range(0, 64, BATCH)), extract)
    assert x.shape == (48, 16) and y.shape == (64, 16) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    return x, y, x.cpu().numpy(), y.cpu().numpy()


def test_device_features_checks():
    G, D = _models(2)
    real = R.synthetic_images(16, IN_SIZE, seed=9).cuda()
    extract = PF.discriminator_features_device(D)
    D.train()
    f = PF.device_features([real[:8], real[8:]], extract)
    assert D.training and torch.equal(f, torch.cat([extract(real[:8]), extract(real[8:])]))
    r = PF.device_features([real[:4].mul(0.5).add(0.5)], lambda b: b.mean(dim=(2, 3)), resize=24, value_range=(0, 1))
    assert r.shape == (4, 3)
    with pytest.raises(ValueError):
        PF.device_features([], extract)
    with pytest.raises(TypeError):
        PF.device_features([real[:8]], lambda b: extract(b).cpu())
    widths = iter((16, 8))
    with pytest.raises(ValueError):
        PF.device_features([real[:8], real[8:]], lambda b: extract(b)[:, :next(widths)])


def test_mmd2_matches_the_restatement(feature_sets):
    x, y, xh, yh = feature_sets
    got = KID.mmd2_unbiased(x, y)
    _assert_estimate(got, xh, yh, "trunk features, 48 x 64")
    assert KID.mmd2_unbiased(x, y) == got
    for kw in (dict(degree=1), dict(degree=2, gamma=0.5, coef0=0.25)):
        _assert_estimate(KID.mmd2_unbiased(x, y, **kw), xh, yh, "trunk features, %r" % kw, **kw)
    # strided rows are read in place: a column slice of a wider tensor, a row slice
    wide = torch.full((48, 21), float("nan"), device=CUDA)
    wide[:, :16] = x
    assert KID.mmd2_unbiased(wide[:, :16], y) == got
    _assert_estimate(KID.mmd2_unbiased(x[5:], y[:2]), xh[5:], yh[:2], "row slices, 43 x 2")
    # the same set twice: every term cancels to rounding (S_xy = S_xx bit for bit, the symmetric form equals the general one)
    same = KID.mmd2_unbiased(x, x.clone())
    assert abs(same - mmd2_unbiased_ref(xh, xh)) <= _bound(xh, xh)
    # the pieces: tile sums and the estimate built from them by hand
    sxx, dx = KID.polykernel_tile_sums(x)
    syy, dy = KID.polykernel_tile_sums(y)
    sxy, none = KID.polykernel_tile_sums(x, y)
    assert none is None and sxx.shape == (1, 1) and syy.shape == (1, 1) and dx.shape == (1,) and sxy.shape == (1, 1)
    assert sxx.dtype == torch.float64 and sxx.is_cuda
    assert KID.mmd2_from_sums(float(sxx.sum()), float(dx.sum()), float(syy.sum()), float(dy.sum()), float(sxy.sum()), 48, 64) == got
    with pytest.raises(ValueError):
        KID.mmd2_unbiased(x[:1], y)
    with pytest.raises(ValueError):
        KID.mmd2_unbiased(x, y[:, :8])
    with pytest.raises(TypeError):
        KID.mmd2_unbiased(x.double(), y.double())


def test_subsets(feature_sets):
    x, y, xh, yh = feature_sets
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = KID.kernel_distance(x, y, num_subsets=3, subset_size=20, seed=5)
    b = KID.kernel_distance(x, y, num_subsets=3, subset_size=20, seed=5)
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    assert a == b and a["mmd2"] == KID.mmd2_unbiased(x, y)
    idx = KID.subset_indices(48, 64, 3, 20, 5)
    for v, (ix, iy) in zip(a["subset_values"], idx):
        _assert_estimate(v, xh[ix.numpy()], yh[iy.numpy()], "subset of 20")
    assert a["subset_mean"] == float(np.mean(a["subset_values"])) and a["subset_std"] == float(np.std(a["subset_values"]))
    assert KID.kernel_distance(x, y, num_subsets=3, subset_size=20, seed=6)["subset_values"] != a["subset_values"]
    # the size is clamped to the smaller set: 48 rows, i.e. all of x in another order and 48 of y's 64
    c = KID.kernel_distance(x, y, num_subsets=2, subset_size=1000, seed=5)
    idx = KID.subset_indices(48, 64, 2, 1000, 5)
    assert len(idx[0][0]) == len(idx[0][1]) == 48
    for v, (ix, iy) in zip(c["subset_values"], idx):
        _assert_estimate(v, xh[ix.numpy()], yh[iy.numpy()], "subset clamped to 48")
    none = KID.kernel_distance(x, y)
    assert none == {"mmd2": a["mmd2"], "subset_mean": None, "subset_std": None}
    with pytest.raises(ValueError):
        KID.kernel_distance(x, y, num_subsets=-1)
    with pytest.raises(ValueError):
        KID.kernel_distance(x, y, num_subsets=2, subset_size=1)


def test_calculate_kid():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(6, 40, 40, 3), dtype=np.uint8)
    b = rng.integers(0, 200, size=(5, 40, 40, 3), dtype=np.uint8)
    extract = lambda x01: torch.cat([x01.mean(dim=(2, 3)), x01[:, :, ::7, ::5].amax(dim=(2, 3))], dim=1)   # (n, 6) on the device
    got = KID.calculate_kid(a, b, extract, batch_size=4)
    # the same batches by hand (a reduction's bits may depend on the batch it runs in)
    fa, fb = (torch.cat([extract(PF.preprocess_images_device(torch.from_numpy(im[i:i + 4]).cuda(), 299)) for i in (0, 4)]).cpu().numpy()
              for im in (a, b))
    assert fa.shape == (6, 6) and fb.shape == (5, 6)
    assert set(got) == {"mmd2", "subset_mean", "subset_std"}
    _assert_estimate(got["mmd2"], fa, fb, "calculate_kid")


def test_metric_ops_is_repeatable_and_leaves_the_networks_alone():
    G, D = _models(3)
    real = R.synthetic_images(32, IN_SIZE, seed=11).cuda()
    metric = KernelDistance(real, n_fake=24, batch_size=BATCH, seed=4)
    G.train(); D.train()
    before = _state(G) + _state(D)
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    v1 = metric.metric_ops(G, D, CUDA)
    v2 = metric.metric_ops(G, D, CUDA)
    assert isinstance(v1, float) and np.isfinite(v1) and v1 == v2
    assert metric.last == {"mmd2": v1, "subset_mean": None, "subset_std": None}
    assert metric._real_stats is None                        # the extractor moves with training: nothing is cached
    assert G.training and D.training
    assert all(torch.equal(a, b) for a, b in zip(before, _state(G) + _state(D))), "running statistics / parameters moved"
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    # the host estimate from fid.device_features of the same batches
    extract = PF.discriminator_features_device(D)
    with torch.no_grad():
        G.eval()
        fake = list(metric._fake_batches(G, metric.noise.cuda()))
        G.train()
    assert [tuple(f.shape) for f in fake] == 3 * [(BATCH, 3, IN_SIZE, IN_SIZE)]
    xf = PF.device_features(fake, extract).cpu().numpy()
    yf = PF.device_features((real[i:i + BATCH] for i in range(0, 32, BATCH)), extract).cpu().numpy()
    assert xf.shape == (24, 16) and yf.shape == (32, 16)
    _assert_estimate(v1, xf, yf, "KernelDistance.metric_ops")
    # subsets: the logged score is their mean, the same at every evaluation
    sub = KernelDistance(real, n_fake=24, batch_size=BATCH, seed=4, num_subsets=4, subset_size=16)
    s1 = sub.metric_ops(G, D, CUDA)
    assert s1 == sub.last["subset_mean"] and sub.last["mmd2"] == v1 and len(sub.last["subset_values"]) == 4
    assert sub.metric_ops(G, D, CUDA) == s1
    # a fixed extractor: resized to 299 first, the real features cached after the first call
    fixed = KernelDistance(real[:6], extractor=lambda x01: x01.mean(dim=(2, 3)), batch_size=3, seed=1)
    f1 = fixed.metric_ops(G, D, CUDA)
    assert torch.is_tensor(fixed._real_stats) and fixed._real_stats.shape == (6, 3) and fixed.metric_ops(G, D, CUDA) == f1
    fixed.set_real(real[6:12])
    assert fixed._real_stats is None


def test_the_real_set_against_itself_is_not_positive():
    """x = y: mmd2 = 2 (S - m D) / (m^2 (m - 1)) with S the sum of the whole Gram matrix and D of its diagonal.  The polynomial
    kernel with coef0 >= 0 is positive semi-definite, so k_ij <= (k_ii + k_jj) / 2 and S <= m D: the unbiased estimate of a set
    against itself is never positive (and not zero unless all rows coincide)."""
    from test_metrics_gpu import _RealAsFake
    G, D = _models(5)
    real = R.synthetic_images(32, IN_SIZE, seed=12).cuda()
    other = KernelDistance(real, batch_size=BATCH, seed=1).metric_ops(G, D, CUDA)
    same = KernelDistance(real, batch_size=BATCH, seed=1).metric_ops(_RealAsFake(real), D, CUDA)
    print("d(real, real) %.3g, d(fake, real) %.3g" % (same, other))
    feats = PF.device_features((real[i:i + BATCH] for i in range(0, 32, BATCH)), PF.discriminator_features_device(D)).cpu().numpy()
    _assert_estimate(same, feats, feats, "the real set against itself")
    assert same <= _bound(feats, feats)


# ------------------------------------------------------------------ the Trainer
def _loader():
    imgs = R.synthetic_images(2 * BATCH, IN_SIZE, seed=5)
    return DataLoader(TensorDataset(imgs, torch.zeros(2 * BATCH)), batch_size=BATCH)


def _trainer(tmp_path, tag, metrics):
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    return P.Trainer(network(), losses, metrics_list=metrics, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4, epochs=2,
                     recon=str(tmp_path / ("img" + tag)), nrow=2)


def _real():
    return R.synthetic_images(16, IN_SIZE, seed=21).cuda()


def test_observer_changes_nothing(tmp_path):
    """Two trainer runs from the same seeds, 2 epochs x 2 iterations, with and without the metric (subsets on: the draws come
    from a private generator): losses, parameters, buffers and Adam moments identical bit for bit; the log has one entry per
    epoch in the first run and does not exist in the second."""
    res = {}
    for with_metric in (True, False):
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        metrics = [KernelDistance(_real(), batch_size=BATCH, seed=8, num_subsets=2, subset_size=8)] if with_metric else None
        tr = _trainer(tmp_path, "m" if with_metric else "p", metrics)
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
    assert list(on[3]) == ["KernelDistance"] and len(on[3]["KernelDistance"]) == 2 and off[3] == {}
    assert all(isinstance(v, float) and np.isfinite(v) for v in on[3]["KernelDistance"])
    assert on[4:] == off[4:]


def test_both_metrics_are_logged_and_survive_a_checkpoint(tmp_path):
    torch.manual_seed(0)
    real = _real()
    tr = _trainer(tmp_path, "a", [FrechetDistance(real, batch_size=BATCH, seed=8), KernelDistance(real, batch_size=BATCH, seed=8)])
    tr(_loader())
    assert sorted(tr.metric_logs) == ["FrechetDistance", "KernelDistance"]
    assert all(len(v) == 2 and all(isinstance(e, float) and np.isfinite(e) for e in v) for v in tr.metric_logs.values())
    # the Frechet distance next to the kernel distance is the one it is alone: same real set, same seed, same noise
    torch.manual_seed(0)
    alone = _trainer(tmp_path, "f", [FrechetDistance(real, batch_size=BATCH, seed=8)])
    alone(_loader())
    assert alone.metric_logs["FrechetDistance"] == tr.metric_logs["FrechetDistance"]
    # an epoch's checkpoint is written before its evaluation (torchgan's order): the file of epoch 2 holds epoch 1's values
    logs = {k: v[:1] for k, v in tr.metric_logs.items()}
    path = str(tmp_path / "gana1.model")
    with_metric = _trainer(tmp_path, "b", [KernelDistance(real, batch_size=BATCH, seed=8)])
    with_metric.load_model(load_path=path)
    assert with_metric.metric_logs == logs and with_metric.start_epoch == 2
    without = _trainer(tmp_path, "c", None)
    without.load_model(load_path=path)
    assert without.metric_logs == logs and without.metrics == {}
    # the loaded trainer with the metric goes on evaluating
    with_metric.epochs = 3
    with_metric(_loader())
    assert len(with_metric.metric_logs["KernelDistance"]) == 2 and with_metric.metric_logs["KernelDistance"][0] == logs["KernelDistance"][0]
    assert with_metric.metric_logs["FrechetDistance"] == logs["FrechetDistance"]
