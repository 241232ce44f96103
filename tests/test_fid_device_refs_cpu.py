"""The device-side Frechet-distance evaluation, checked without a GPU: the numpy restatements of the two kernels
(tests/fid_device_refs.py) against their own definitions and against the product's host path, FeatureMoments' finishing
formula against np.cov, the Trainer's per-epoch metric plumbing on the CPU device with a dummy EvaluationMetric, the
FrechetDistance pickle and the CLI flags."""
import pickle

import numpy as np
import pytest
import torch
import torch.nn as nn

import rna_gan_amd as P
from rna_gan_amd import fid as FID
from rna_gan_amd import losses as L
from rna_gan_amd.metrics import EvaluationMetric, FrechetDistance
from rna_gan_amd.trainer import Trainer
from fid_device_refs import RESIZE_BOUND, axis_taps, moments_int, moments_ld, resize_ref, tap_f32, tap_u8


def _network():
    """the tiny networks of tests/test_checkpoint_compat_cpu.py"""
    return {
        "generator": {"name": P.DCGANGenerator,
                      "args": dict(encoding_dims=16, out_size=32, out_channels=3, step_channels=4,
                                   nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh()),
                      "optimizer": {"name": torch.optim.Adam, "args": {"lr": 1e-4, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": dict(in_size=32, in_channels=3, step_channels=4,
                                       nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2)),
                          "optimizer": {"name": torch.optim.Adam, "args": {"lr": 4e-4, "betas": (0.5, 0.999)}}}}


def _plugins():
    return [L.WassersteinGeneratorLoss(), L.WassersteinDiscriminatorLoss(clip=(-0.01, 0.01)), L.WassersteinGradientPenalty()]


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _ulp_below(size):
    """ulp of the largest fp32 source coordinate of an axis of `size` taps (coordinates stay below size): 2^-16 at 256"""
    return float(np.spacing(np.nextafter(np.float32(size), np.float32(0))))


# ------------------------------------------------------------------ resize restatement
def test_taps():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(tap_u8(v), (torch.arange(256).float() / 255).numpy())            # the host path's division
    assert tap_u8(v).dtype == np.float32 and tap_u8(v)[0] == 0.0 and tap_u8(v)[255] == 1.0
    g = np.random.default_rng(0).uniform(-1, 1, 1000).astype(np.float32)
    assert np.array_equal(tap_f32(g, 1.0, 0.0), g)
    assert np.array_equal(tap_f32(g, 0.5, 0.5), g * np.float32(0.5) + np.float32(0.5))
    assert tap_f32(np.float32([-1, 1]), 0.5, 0.5).tolist() == [0.0, 1.0]


@pytest.mark.parametrize("n", [1, 2, 8, 13, 256])
def test_identity_axis_has_zero_weights(n):
    i0, i1, lam = axis_taps(n, n)
    assert np.array_equal(i0, np.arange(n)) and np.all(lam == 0.0) and lam.dtype == np.float32
    assert np.array_equal(i1, np.minimum(np.arange(n) + 1, n - 1))


@pytest.mark.parametrize("n_in,n_out", [(1, 3), (2, 5), (3, 4), (5, 7), (7, 5), (40, 17), (24, 11), (16, 19), (13, 299), (256, 299)])
def test_axis_taps_stay_inside(n_in, n_out):
    i0, i1, lam = axis_taps(n_in, n_out)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(i1 - i0 <= 1) and np.all(i1 >= i0)
    assert np.all(lam >= 0.0) and np.all(lam < 1.0)
    assert i0[0] == 0 and lam[0] == 0.0 if n_out >= n_in else True                       # the lower clamp (upscaling)


def test_identity_sizes_reproduce_the_taps():
    t = tap_u8(_u8((2, 3, 8, 8), 1))
    assert np.array_equal(resize_ref(t, 8, 8), t.astype(np.float64))


@pytest.mark.parametrize("hw,out", [((1, 1), (3, 3)), ((2, 3), (5, 4)), ((5, 7), (7, 5)), ((40, 24), (17, 11)), ((13, 9), (299, 299))])
def test_outputs_of_unit_range_inputs_stay_in_it(hw, out):
    t = tap_u8(_u8((2, 3) + hw, 2))
    y = resize_ref(t, *out)
    assert y.shape == (2, 3) + out and y.min() >= 0.0 and y.max() <= 1.0
    assert y.min() >= t.min() and y.max() <= t.max()                                     # a convex combination of taps
    ones = resize_ref(np.ones((1, 3) + hw, dtype=np.float32), *out)
    assert ones.min() >= 1.0 - RESIZE_BOUND and ones.max() <= 1.0


@pytest.mark.parametrize("size", [256, 512])
def test_restatement_against_the_host_preprocess(size):
    """The product's host path resizes with torch's interpolate, whose source coordinates are fp32.  Tolerance:
    4 ulp_fp32(max(H, W)) -- two axes x at most two roundings of an fp32 coordinate of that magnitude x tap differences
    <= 1: 6.1e-5 at 256, 1.2e-4 at 512."""
    img = _u8((1, size, size, 3), 3)
    host = FID.preprocess_images(img).numpy().astype(np.float64)
    ref = resize_ref(tap_u8(np.transpose(img, (0, 3, 1, 2))), 299, 299)
    err = float(np.abs(host - ref).max())
    tol = 4 * _ulp_below(size)
    print("host preprocess_images vs fp64-coordinate restatement at %d -> 299: max |diff| %.3g (tolerance %.3g)" % (size, err, tol))
    assert err <= tol


def test_host_preprocess_on_float_images_too():
    img = np.random.default_rng(4).uniform(0, 1, (1, 40, 24, 3)).astype(np.float32)
    host = FID.preprocess_images(img).numpy().astype(np.float64)
    ref = resize_ref(tap_f32(np.transpose(img, (0, 3, 1, 2)), 1.0, 0.0), 299, 299)
    assert float(np.abs(host - ref).max()) <= 4 * _ulp_below(40)


# ------------------------------------------------------------------ moments
def test_moment_restatements_agree_on_integers():
    x = np.random.default_rng(5).integers(-2047, 2048, size=(37, 17)).astype(np.float32)
    s1, s2 = moments_int(x)
    l1, l2, a2, a1 = moments_ld(x)
    assert np.array_equal(l1, s1.astype(np.longdouble)) and np.array_equal(l2, s2.astype(np.longdouble))
    assert np.array_equal(s2, s2.T) and np.all(a2 >= np.abs(l2)) and np.all(a1 >= np.abs(l1))
    assert float(np.abs(s2).max()) < 2.0 ** 53                                           # exact in fp64 as well


@pytest.mark.parametrize("n,F", [(37, 48), (2048, 256)])
def test_finishing_formula_against_np_cov(n, F):
    """FeatureMoments.finish fed the exact raw moments (rounded once to fp64) against np.cov / mean on float64."""
    g = torch.Generator().manual_seed(n + F)
    x = (torch.rand(n, F, generator=g) * torch.rand(F, generator=g) * 0.5).numpy()       # pool-feature-like: non-negative
    s1, s2, _, _ = moments_ld(x)
    mu, sigma = FID.FeatureMoments.finish(s1.astype(np.float64), s2.astype(np.float64), n)
    want_mu, want_sigma = FID.activation_statistics(x)
    err = float(np.abs(sigma - want_sigma).max())
    scale = float(np.abs(want_sigma).max())
    print("finish vs np.cov at (%d, %d): max |diff| %.3g, max |cov| %.3g" % (n, F, err, scale))
    assert err <= 1e-12 * scale
    assert float(np.abs(mu - want_mu).max()) <= 1e-12 * float(np.abs(want_mu).max())
    assert np.array_equal(sigma, sigma.T)


def test_finish_refuses_fewer_than_two_rows():
    for n in (0, 1):
        with pytest.raises(ValueError):
            FID.FeatureMoments.finish(np.zeros(3), np.zeros((3, 3)), n)


def test_device_entry_points_refuse_host_tensors():
    with pytest.raises(TypeError):
        FID.preprocess_images_device(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(TypeError):
        FID.device_statistics([torch.zeros(2, 3, 8, 8)], lambda b: np.zeros((2, 4)))


def test_on_device_keyword_reaches_calculate_fid(monkeypatch):
    seen = []
    monkeypatch.setattr(FID, "calculate_fid", lambda r, f, e, b, on_device=False: seen.append((b, on_device)) or 1.0)
    FID.fid_protocol(lambda: None, None, None, iterations=2, batch_size=3, on_device=True)
    FID.fid_protocol(lambda: None, None, None, iterations=1)
    assert seen == [(3, True), (3, True), (2, False)]


# ------------------------------------------------------------------ Trainer plumbing (CPU device, dummy metric)
class CountingMetric(EvaluationMetric):
    def __init__(self):
        super().__init__()
        self.seen = []

    def metric_ops(self, generator, discriminator, device, epochs):
        self.seen.append((generator, discriminator, device, epochs))
        return 10.0 * len(self.seen) + epochs


class RenamedMetric(EvaluationMetric):
    def __init__(self):
        super().__init__()
        self.set_arg_map({"net": "generator", "count": "ncritic"})
        self.seen = []

    def metric_ops(self, net, count):
        self.seen.append((net, count))
        return float(count)


def _trainer(tmp_path, name, metrics, **kw):
    return Trainer(_network(), _plugins(), metrics_list=metrics, device=torch.device("cpu"), checkpoints=str(tmp_path / name),
                   recon=None, **kw)


def test_metric_logs_one_entry_per_epoch_and_arguments_by_name(tmp_path, capsys):
    a, b = CountingMetric(), RenamedMetric()
    tr = _trainer(tmp_path, "gan", [a, b], epochs=3, ncritic=5, prefetch=False)
    assert tr.metric_logs == {"CountingMetric": [], "RenamedMetric": []}
    tr.generator.train(); tr.discriminator.eval()
    for epoch in range(3):
        tr.eval_ops(epoch)
    assert tr.metric_logs == {"CountingMetric": [13.0, 23.0, 33.0], "RenamedMetric": [5.0, 5.0, 5.0]}
    assert all(s[0] is tr.generator and s[1] is tr.discriminator and s[2] == tr.device and s[3] == 3 for s in a.seen)
    assert all(s[0] is tr.generator and s[1] == 5 for s in b.seen)
    assert tr.generator.training and not tr.discriminator.training                       # modes are put back
    out = capsys.readouterr().out
    assert "CountingMetric : 13.0" in out and "RenamedMetric : 5.0" in out


def test_eval_ops_restores_modes_when_a_metric_flips_them(tmp_path):
    class Flipper(EvaluationMetric):
        def metric_ops(self, generator, discriminator):
            generator.eval(); discriminator.train()
            return 0.0
    tr = _trainer(tmp_path, "gan", [Flipper()])
    tr.generator.train(); tr.discriminator.eval()
    tr.eval_ops(0)
    assert tr.generator.training and not tr.discriminator.training


def test_train_calls_eval_ops_once_per_epoch(tmp_path):
    """The loop itself, on an empty loader (no train_op can run on the CPU device): one value per epoch."""
    m = CountingMetric()
    tr = _trainer(tmp_path, "gan", [m], epochs=2, prefetch=False)
    tr.train([])
    assert tr.metric_logs["CountingMetric"] == [12.0, 22.0]


def test_no_metrics_behaves_as_before(tmp_path):
    tr = _trainer(tmp_path, "gan", None, epochs=1, prefetch=False)
    assert tr.metrics == {} and tr.metric_logs == {}
    tr.eval_ops(0)
    tr.train([])
    assert tr.metric_logs == {}


def test_checkpoint_round_trip_keeps_the_log(tmp_path):
    real = torch.zeros(4, 3, 32, 32, dtype=torch.uint8)
    tr = _trainer(tmp_path, "gan", [CountingMetric(), FrechetDistance(real)], epochs=2)
    tr.metric_logs["CountingMetric"] += [1.5, 2.5]
    tr.metric_logs["FrechetDistance"] += [7.0]
    tr.save_model(1)
    path = str(tmp_path / "gan0.model")
    with_metric = _trainer(tmp_path, "a", [FrechetDistance(real), CountingMetric()])
    with_metric.load_model(load_path=path)
    assert with_metric.metric_logs == {"CountingMetric": [1.5, 2.5], "FrechetDistance": [7.0]}
    other = _trainer(tmp_path, "b", [RenamedMetric()])
    other.load_model(load_path=path)                                                     # a live metric the file never saw
    assert other.metric_logs == {"CountingMetric": [1.5, 2.5], "FrechetDistance": [7.0], "RenamedMetric": []}
    without = _trainer(tmp_path, "c", None)
    without.load_model(load_path=path)
    assert without.metric_logs == {"CountingMetric": [1.5, 2.5], "FrechetDistance": [7.0]} and without.start_epoch == 2
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["metric_objects"]["FrechetDistance"].real is None                          # settings only


def test_frechet_distance_pickles_settings_only():
    real = torch.randint(0, 256, (64, 3, 64, 64), dtype=torch.uint8)
    m = FrechetDistance(real, n_fake=48, seed=3, batch_size=16, encoding_dims=128)
    m.set_arg_map({"generator": "generator_ema"})
    m._real_stats = (np.zeros(2048), np.zeros((2048, 2048)), 64)
    blob = pickle.dumps(m)
    assert len(blob) < 64 * 1024, len(blob)
    back = pickle.loads(blob)
    assert (back.n_fake, back.seed, back.batch_size, back.extractor) == (48, 3, 16, "discriminator")
    assert back.arg_map == {"generator": "generator_ema"}
    assert back.real is None and back.noise is None and back._real_stats is None
    with pytest.raises(RuntimeError):
        back.metric_ops(None, None, torch.device("cpu"))
    assert pickle.loads(pickle.dumps(FrechetDistance(real, extractor=lambda x: x))).extractor == "callable"


def test_pickled_state_of_every_metric_keeps_its_keys():
    """the keys a checkpoint holds per metric, as literals: a checkpoint written by an earlier version must go on loading"""
    from rna_gan_amd.metrics import ConditioningFidelity, KernelDistance, Memorisation, PrecisionRecall, TissueYield
    real = torch.zeros(8, 3, 32, 32, dtype=torch.uint8)
    cases = [
        (FrechetDistance(real), {"arg_map", "n_fake", "seed", "batch_size", "extractor"}),
        (KernelDistance(real), {"arg_map", "n_fake", "seed", "batch_size", "extractor", "num_subsets", "subset_size", "degree",
                                "gamma", "coef0"}),
        (PrecisionRecall(real), {"arg_map", "n_fake", "seed", "batch_size", "extractor", "nearest_k", "report", "history"}),
        (TissueYield(8), {"arg_map", "n_fake", "seed", "batch_size", "min_tissue", "fraction", "luma_range", "rgb_min", "dilate",
                          "percentiles", "history"}),
        (ConditioningFidelity(real, torch.arange(8) % 2, torch.zeros(2, 5), None),
         {"arg_map", "tiles_per_patient", "seed", "batch_size", "group", "center", "report", "extractor", "history"}),
        (Memorisation(real, 8), {"arg_map", "n_fake", "seed", "batch_size", "factor", "k", "d4", "history"}),
    ]
    for metric, keys in cases:
        state = metric.__getstate__()
        assert set(state) == keys, type(metric).__name__
        back = pickle.loads(pickle.dumps(metric))
        assert type(back) is type(metric) and back.__getstate__() == state, type(metric).__name__


def test_frechet_distance_noise_is_private_and_repeatable():
    real = torch.zeros(8, 3, 32, 32, dtype=torch.uint8)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    a = FrechetDistance(real, seed=5, encoding_dims=16)
    b = FrechetDistance(real, seed=5)

    class G:
        encoding_dims = 16
    zb = b._noise_for(G(), torch.device("cpu"))
    assert torch.equal(torch.get_rng_state(), before)                                    # the global generator was not used
    assert a.noise.shape == (8, 16) and torch.equal(a.noise, zb) and torch.equal(b._noise_for(G(), torch.device("cpu")), zb)
    assert not torch.equal(FrechetDistance(real, seed=6, encoding_dims=16).noise, a.noise)
    given = torch.ones(8, 16)
    assert torch.equal(FrechetDistance(real, noise=given)._noise_for(G(), torch.device("cpu")), given)
    calls = []
    c = FrechetDistance(real, noise=lambda n: calls.append(n) or torch.zeros(n, 16))
    c._noise_for(G(), torch.device("cpu")); c._noise_for(G(), torch.device("cpu"))
    assert calls == [8, 8]
    with pytest.raises(ValueError):
        FrechetDistance(real, noise=torch.ones(7, 16))
    with pytest.raises(ValueError):
        FrechetDistance(real, extractor="inception")
    with pytest.raises(ValueError):
        FrechetDistance(real[:1])


# ------------------------------------------------------------------ CLI
def test_cli_flags(tmp_path, capsys):
    import histopathology_gan as H
    base = ["--config", "c.json"]
    a = H.parse_args(base)
    assert a.fd_samples == 0 and a.fd_extractor == "discriminator"
    a = H.parse_args(base + ["--fd_samples", "2048"])
    assert a.fd_samples == 2048
    weights = tmp_path / "inception.pt"
    weights.write_bytes(b"x")
    a = H.parse_args(base + ["--fd_samples", "64", "--fd_extractor", str(weights)])
    assert a.fd_extractor == str(weights)
    for bad in (["--fd_samples", "-1"], ["--fd_samples", "1"], ["--fd_samples", "many"],
                ["--fd_samples", "8", "--fd_extractor", str(tmp_path / "absent.pt")], ["--fd_extractor", "inception"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()
