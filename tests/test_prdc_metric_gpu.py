"""Precision / recall / density / coverage end to end (rna_gan_amd.prdc, rna_gan_amd.metrics.PrecisionRecall, Trainer.eval_ops,
the CLI's --pr_samples) with the tiny networks of tests/test_metrics_gpu.py: in_size 32, step_channels 4 (F = 16 trunk
features), encoding_dims 16, batch 8.

prdc.prdc on integer feature sets EQUALS the restatement of tests/prdc_refs.py: every d2 is an exact integer, so radii, hits
and the four ratios (one IEEE division each, of the same integers) are the same bits on both sides."""
import pickle

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from oracle import ref_cpu as R
from rna_gan_amd import fid as PF
from rna_gan_amd import prdc as PR
from rna_gan_amd.metrics import KernelDistance, PrecisionRecall
from prdc_refs import hits_ref, integer_case, prdc_ref, radii2_ref
from test_metrics_gpu import BATCH, IN_SIZE, _models, _state, network

CUDA = torch.device("cuda:0")
FOUR = ("precision", "recall", "density", "coverage")


def _dev(x):
    return torch.from_numpy(np.array(x)).to(CUDA)


def _assert_four(d):
    assert sorted(d) == sorted(FOUR) and all(isinstance(v, float) for v in d.values())
    assert all(0.0 <= d[key] <= 1.0 for key in ("precision", "recall", "coverage")) and d["density"] >= 0.0, d


# ------------------------------------------------------------------ rna_gan_amd.prdc
@pytest.mark.parametrize("m,n,F", [(130, 70, 70), (65, 33, 33)])
def test_prdc_equals_the_restatement_on_integer_sets(m, n, F):
    xh, yh = integer_case(m, n, F, seed=m + F)
    x, y = _dev(xh), _dev(yh)
    for k in (1, 3, 5):
        want = prdc_ref(xh, yh, k)
        got = PR.prdc(x, y, k=k)
        print("k=%d %r" % (k, got))
        _assert_four(got)
        assert got == want, (k, got, want)
        radii = PR.knn_radii2(x, k)
        assert radii.dtype == torch.float64 and radii.is_cuda and np.array_equal(radii.cpu().numpy(), radii2_ref(xh, k))
        assert PR.prdc(x, y, k=k, real_radii2=radii) == want, "real_radii2 passed in"
    assert PR.precision_recall(x, y) == (prdc_ref(xh, yh, 3)["precision"], prdc_ref(xh, yh, 3)["recall"])
    assert PR.density_coverage(x, y) == (prdc_ref(xh, yh, 5)["density"], prdc_ref(xh, yh, 5)["coverage"])
    # the pieces
    ry = radii2_ref(yh, 3)
    count, mind2 = PR.radius_hits(x, y, _dev(ry))
    wcount, wmin = hits_ref(xh, yh, ry)
    assert count.dtype == torch.int32 and mind2.dtype == torch.float64 and count.is_cuda and mind2.is_cuda
    assert np.array_equal(count.cpu().numpy(), wcount) and np.array_equal(mind2.cpu().numpy(), wmin)
    none, only = PR.radius_hits(x, y)
    assert none is None and torch.equal(only, mind2)


def test_strided_inputs_are_read_in_place(monkeypatch):
    xh, yh = integer_case(65, 33, 33, seed=98)
    want = prdc_ref(xh, yh, 3)
    wide = torch.full((70, 40), float("nan"), device=CUDA)       # a column slice and a row slice of wider / longer tensors
    wide[:65, :33] = _dev(xh)
    tall = torch.full((40, 33), float("nan"), device=CUDA)
    tall[2:35] = _dev(yh)
    xs, ys = wide[:65, :33], tall[2:35]
    assert not xs.is_contiguous() and xs.stride(0) == 40
    copies = []
    real_contiguous = torch.Tensor.contiguous
    monkeypatch.setattr(torch.Tensor, "contiguous", lambda t, *a, **kw: copies.append(tuple(t.shape)) or real_contiguous(t, *a, **kw))
    got = PR.prdc(xs, ys, k=3)
    radii = PR.knn_radii2(xs, 3)
    count, _ = PR.radius_hits(ys, xs, radii)
    monkeypatch.undo()
    assert got == want and not [s for s in copies if len(s) == 2], "a feature set was copied: %r" % copies
    assert np.array_equal(count.cpu().numpy(), hits_ref(yh, xh, radii2_ref(xh, 3))[0])
    # a transposed view has no unit column stride: copied once, the same result
    assert PR.prdc(_dev(xh).t().contiguous().t(), ys, k=3) == want
    x, y = _dev(xh), _dev(yh)
    with pytest.raises(ValueError):
        PR.prdc(x, y, k=0)
    with pytest.raises(ValueError):
        PR.prdc(x, y, k=17)
    with pytest.raises(ValueError):
        PR.prdc(x, y[:5], k=5)                                    # k + 1 rows are needed in both sets
    with pytest.raises(ValueError):
        PR.prdc(x, y[:, :8])
    with pytest.raises(ValueError):
        PR.prdc(x, y, k=3, real_radii2=torch.zeros(64, dtype=torch.float64, device=CUDA))
    with pytest.raises(TypeError):
        PR.prdc(x.double(), y.double())
    # the workspace is one cached buffer per device, grown on demand and reused
    ws = PR._WS[("cuda", 0)]
    PR.prdc(x, y, k=1)
    assert PR._WS[("cuda", 0)] is ws


def test_calculate_prdc():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(6, 40, 40, 3), dtype=np.uint8)
    b = rng.integers(0, 200, size=(5, 40, 40, 3), dtype=np.uint8)
    extract = lambda x01: torch.cat([x01.mean(dim=(2, 3)), x01[:, :, ::7, ::5].amax(dim=(2, 3))], dim=1)   # (n, 6) on the device
    got = PR.calculate_prdc(a, b, extract, batch_size=4, k=2)
    _assert_four(got)
    fa, fb = (torch.cat([extract(PF.preprocess_images_device(torch.from_numpy(im[i:i + 4]).cuda(), 299)) for i in (0, 4)])
              for im in (a, b))
    assert fa.shape == (6, 6) and fb.shape == (5, 6) and got == PR.prdc(fa, fb, k=2)


# ------------------------------------------------------------------ the metric
def test_metric_ops_is_repeatable_and_leaves_the_networks_alone():
    """2 k + 2 = 12 tiles at the default k = 5"""
    G, D = _models(3)
    real = R.synthetic_images(12, IN_SIZE, seed=11).cuda()
    metric = PrecisionRecall(real, batch_size=12, seed=4)
    assert metric.n_fake == 12 and metric.nearest_k == 5 and metric.report == "recall"
    G.train(); D.train()
    before = _state(G) + _state(D)
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    v1 = metric.metric_ops(G, D, CUDA)
    first = dict(metric.last)
    v2 = metric.metric_ops(G, D, CUDA)
    assert isinstance(v1, float) and v1 == v2 == first["recall"] and metric.last == first and metric.history == [first, first]
    _assert_four(first)
    print("PrecisionRecall on 12 + 12 tiles: %r" % first)
    assert metric._real_stats is None and metric._real_radii is None   # the extractor moves with training: nothing is cached
    assert G.training and D.training
    assert all(torch.equal(a, b) for a, b in zip(before, _state(G) + _state(D))), "running statistics / parameters moved"
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state())
    # the same four values from prdc.prdc on fid.device_features of the same batches
    extract = PF.discriminator_features_device(D)
    with torch.no_grad():
        G.eval()
        fake = list(metric._fake_batches(G, metric.noise.cuda()))
        G.train()
    xf = PF.device_features([real], extract)
    yf = PF.device_features(fake, extract)
    assert xf.shape == (12, 16) and yf.shape == (12, 16) and PR.prdc(xf, yf, k=5) == first
    # each report returns its entry of the same evaluation
    for report in FOUR:
        other = PrecisionRecall(real, batch_size=12, seed=4, report=report)
        assert other.metric_ops(G, D, CUDA) == first[report] and other.last == first
    # the real set as the generated set: every row lies in its own ball
    from test_metrics_gpu import _RealAsFake
    same = PrecisionRecall(real, batch_size=12, seed=4, nearest_k=3)
    same.metric_ops(_RealAsFake(real), D, CUDA)
    assert same.last["precision"] == same.last["recall"] == same.last["coverage"] == 1.0 and same.last["density"] >= 1.0
    # a fixed extractor: resized to 299 first, the real features AND their radii cached after the first call
    fixed = PrecisionRecall(real[:6], extractor=lambda x01: x01.mean(dim=(2, 3)), batch_size=3, seed=1, nearest_k=2)
    f1 = fixed.metric_ops(G, D, CUDA)
    feats, radii = fixed._real_stats, fixed._real_radii
    assert torch.is_tensor(feats) and feats.shape == (6, 3) and torch.is_tensor(radii) and radii.shape == (6,)
    assert torch.equal(radii, PR.knn_radii2(feats, 2))
    assert fixed.metric_ops(G, D, CUDA) == f1 and fixed._real_radii is radii and fixed._real_stats is feats
    fixed.set_real(real[6:12])
    assert fixed._real_stats is None and fixed._real_radii is None


def test_pickle_keeps_settings_and_history_and_set_real_restores_evaluation():
    G, D = _models(4)
    real = R.synthetic_images(BATCH, IN_SIZE, seed=13).cuda()
    metric = PrecisionRecall(real, batch_size=BATCH, seed=2, nearest_k=3, report="coverage")
    v = metric.metric_ops(G, D, CUDA)
    blob = pickle.dumps(metric)
    assert len(blob) < 16 * 1024
    back = pickle.loads(blob)
    assert (back.nearest_k, back.report, back.seed, back.batch_size, back.n_fake) == (3, "coverage", 2, BATCH, BATCH)
    assert back.history == metric.history == [metric.last] and back.last is None
    assert back.real is None and back.noise is None and back._real_stats is None and back._real_radii is None
    with pytest.raises(RuntimeError, match="set_real"):
        back.metric_ops(G, D, CUDA)
    back.set_real(real)
    assert back.metric_ops(G, D, CUDA) == v                      # the same private noise from the same seed
    assert back.history == [metric.last, metric.last]


# ------------------------------------------------------------------ the Trainer
def _loader():
    imgs = R.synthetic_images(2 * BATCH, IN_SIZE, seed=5)
    return DataLoader(TensorDataset(imgs, torch.zeros(2 * BATCH)), batch_size=BATCH)


def _trainer(tmp_path, tag, metrics, epochs=2):
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    return P.Trainer(network(), losses, metrics_list=metrics, checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4, epochs=epochs,
                     recon=str(tmp_path / ("img" + tag)), nrow=2)


def _real():
    return R.synthetic_images(BATCH, IN_SIZE, seed=21).cuda()      # 2 k + 2 tiles at k = 3


def test_observer_changes_nothing_and_the_log_survives_a_checkpoint(tmp_path):
    """Two trainer runs from the same seeds, 2 epochs x 2 iterations, with and without the metric: losses, parameters, buffers
    and Adam moments identical bit for bit; one float per epoch under metric_logs["PrecisionRecall"], all four values per epoch
    in the metric's history, both in the checkpoint."""
    res = {}
    for with_metric in (True, False):
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        metrics = [PrecisionRecall(_real(), batch_size=BATCH, seed=8, nearest_k=3, report="precision")] if with_metric else None
        tr = _trainer(tmp_path, "m" if with_metric else "p", metrics)
        tr(_loader())
        torch.cuda.synchronize()
        og, od = tr.optimizer_generator, tr.optimizer_discriminator
        res[with_metric] = (tr.loss_logs, _state(tr.generator) + _state(tr.discriminator),
                            [og._m.clone(), og._v.clone(), od._m.clone(), od._v.clone(), og._step_dev.clone()], tr.metric_logs,
                            tr.generator.training, tr.discriminator.training)
        if with_metric:
            live = tr.metrics["PrecisionRecall"]
    on, off = res[True], res[False]
    assert on[0] == off[0] and all(len(v) == 4 for v in on[0].values())
    for k in (1, 2):
        assert len(on[k]) == len(off[k])
        for a, b in zip(on[k], off[k]):
            assert torch.equal(a, b)
    log = on[3]["PrecisionRecall"]
    assert list(on[3]) == ["PrecisionRecall"] and len(log) == 2 and off[3] == {} and on[4:] == off[4:]
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in log)
    assert len(live.history) == 2 and [h["precision"] for h in live.history] == log
    for h in live.history:
        _assert_four(h)
    # an epoch's checkpoint is written before its evaluation (torchgan's order): the file of epoch 2 holds epoch 1's values
    path = str(tmp_path / "ganm1.model")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["metric_logs"] == {"PrecisionRecall": log[:1]}
    saved = ck["metric_objects"]["PrecisionRecall"]
    assert saved.real is None and saved.history == live.history[:1] and (saved.nearest_k, saved.report) == (3, "precision")
    again = _trainer(tmp_path, "b", [PrecisionRecall(_real(), batch_size=BATCH, seed=8, nearest_k=3, report="precision")], epochs=3)
    again.load_model(load_path=path)
    assert again.metric_logs == {"PrecisionRecall": log[:1]} and again.start_epoch == 2
    assert again.metrics["PrecisionRecall"].history == live.history[:1] and again.metrics["PrecisionRecall"].real is not None
    without = _trainer(tmp_path, "c", None)
    without.load_model(load_path=path)
    assert without.metric_logs == {"PrecisionRecall": log[:1]} and without.metrics == {}
    again(_loader())                                             # the loaded trainer goes on evaluating and logging
    assert len(again.metric_logs["PrecisionRecall"]) == 2 and again.metric_logs["PrecisionRecall"][0] == log[0]
    assert len(again.metrics["PrecisionRecall"].history) == 2


def test_three_metrics_side_by_side(tmp_path):
    from rna_gan_amd.metrics import FrechetDistance
    torch.manual_seed(0)
    real = R.synthetic_images(16, IN_SIZE, seed=21).cuda()
    tr = _trainer(tmp_path, "a", [FrechetDistance(real, batch_size=BATCH, seed=8), KernelDistance(real, batch_size=BATCH, seed=8),
                                  PrecisionRecall(real, batch_size=BATCH, seed=8)], epochs=1)
    tr(_loader())
    assert sorted(tr.metric_logs) == ["FrechetDistance", "KernelDistance", "PrecisionRecall"]
    assert all(len(v) == 1 and isinstance(v[0], float) and np.isfinite(v[0]) for v in tr.metric_logs.values())
    torch.manual_seed(0)
    alone = _trainer(tmp_path, "k", [KernelDistance(real, batch_size=BATCH, seed=8)], epochs=1)
    alone(_loader())
    assert alone.metric_logs["KernelDistance"] == tr.metric_logs["KernelDistance"]


# ------------------------------------------------------------------ CLI
def test_cli_smoke(capsys):
    import histopathology_gan as H
    base = ["--config", "c.json", "--loss_type", "wgan", "--seed", "5"]
    for bad in (["--pr_samples", "5"], ["--pr_samples", "3", "--pr_k", "3"], ["--pr_samples", "2", "--pr_k", "3"]):
        with pytest.raises(SystemExit):
            H.parse_args(base + bad)
    capsys.readouterr()
    args = H.parse_args(base + ["--kid_samples", "8", "--pr_samples", "8", "--pr_k", "3", "--pr_report", "coverage"])
    ds = H.SyntheticTiles(8, IN_SIZE, 4, False, 0)
    holder = {}
    kd = H.build_kid_metric(args, ds, [], CUDA, holder)
    pr = H.build_pr_metric(args, ds, [], CUDA, holder)
    assert isinstance(pr, PrecisionRecall) and pr.real is kd.real and pr.real.is_cuda and pr.real.shape == (8, 3, IN_SIZE, IN_SIZE)
    assert pr.noise is kd.noise and pr.extractor == kd.extractor == "discriminator"
    assert (pr.nearest_k, pr.report, pr.seed, pr.batch_size, pr.n_fake) == (3, "coverage", 5, 8, 8)
    G, D = _models(6)
    v = pr.metric_ops(G, D, CUDA)
    _assert_four(pr.last)
    assert v == pr.last["coverage"] and np.isfinite(kd.metric_ops(G, D, CUDA))
