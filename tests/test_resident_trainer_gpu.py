"""Trainer.train over a resident set (rna_gan_amd.resident) on the GPU: what every loss plugin finds in ``real_inputs``.

A loss stub records the image of every batch, its side data and the loader transform's codes at that moment; the yardstick is the
numpy restatement of tests/resident_refs.py applied to the set's own uint8 tiles in the loader's order, bit for bit.  The networks
and the stub are those of tests/test_augment_trainer_gpu.py, restated here: out_size 16, 4 step channels (nothing of them runs
under the stub); two tests run real ``wgan`` and ``wganvae`` iterations on them."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import Adam
from torch.utils.data import DataLoader, Dataset, Sampler

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from rna_gan_amd import losses as PL
from rna_gan_amd.augment import InputTransform
from rna_gan_amd.resident import DeviceTileLoader, DeviceTileSet
from resident_refs import epoch_order_ref, gather_transform_ref

S, BATCH, TILES, G = 16, 4, 14, 64          # three full batches per epoch; two tiles of each order stay out
DEV = "cuda:0"
RECORDS = []                                # (image, codes or None, rna or None, labels or None) per train_ops call of the stub
CODES_OF = [None]                           # the transform whose last_codes the stub reads (the loader's, or the Trainer's)

_RNG = np.random.default_rng(53)
_U8 = _RNG.integers(0, 256, size=(TILES, 3, S, S), dtype=np.uint8)
_RNA = _RNG.standard_normal((5, G)).astype(np.float32)
_ROW_OF = (np.arange(TILES) % 5).astype(np.int32)
_LABELS = np.arange(TILES, dtype=np.float32)
for _a in (_U8, _RNA, _ROW_OF, _LABELS):
    _a.setflags(write=False)


@pytest.fixture(autouse=True)
def _restore_plugin_globals():
    """Trainer.train sets losses.TRAINER_LOOKAHEAD for its own plugin list (the D-loss plugin then draws the penalty's noise) and
    leaves it set; test files that run later call the plugins directly under seeds of their own and must find it as it was."""
    was = PL.TRAINER_LOOKAHEAD[0], PL._NEXT_NOISE[0]
    yield
    PL.TRAINER_LOOKAHEAD[0], PL._NEXT_NOISE[0] = was


def _network(enc=64):
    return {
        "generator": {"name": P.DCGANGenerator,
                      "args": {"encoding_dims": enc, "out_channels": 3, "step_channels": 4, "out_size": S,
                               "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.Tanh()},
                      "optimizer": {"name": Adam, "args": {"lr": 0.0001, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": {"in_size": S, "in_channels": 3, "step_channels": 4,
                                   "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.LeakyReLU(0.2)},
                          "optimizer": {"name": Adam, "args": {"lr": 0.0004, "betas": (0.5, 0.999)}}},
    }


class RecordRealInputs(PL.DiscriminatorLoss):
    """What a loss plugin sees: train_ops resolves ``real_inputs`` and ``labels`` by name."""

    def train_ops(self, real_inputs, labels):
        rna = None
        if isinstance(real_inputs, dict):
            image, rna, labels = real_inputs["image"], real_inputs["rna_data"], real_inputs["labels"]
        else:
            image = real_inputs
        assert image.dtype == torch.float32 and image.is_contiguous() and image.is_cuda
        tf = CODES_OF[0]
        codes = None if tf is None or tf.last_codes is None else tf.last_codes.copy()
        RECORDS.append((image.detach().cpu().numpy().copy(), codes, None if rna is None else rna.cpu().numpy().copy(),
                        None if labels is None else labels.cpu().numpy().copy()))
        return 0.0


def _tileset(form):
    t = torch.from_numpy(_U8.copy())
    if form == "tensor":
        return DeviceTileSet.from_tensors(t, device=DEV)
    if form == "tuple":
        return DeviceTileSet.from_tensors(t, labels=torch.from_numpy(_LABELS.copy()), device=DEV)
    return DeviceTileSet.from_tensors(t, rna=torch.from_numpy(_RNA.copy()), row_of=torch.from_numpy(_ROW_OF.copy()),
                                      labels=torch.from_numpy(_LABELS.copy()), device=DEV)


def _resident(form, augment, seed=4, batch=BATCH):
    tf = InputTransform(augment=augment, seed=seed, rank=0)
    return DeviceTileLoader(_tileset(form), batch, transform=tf, seed=seed, rank=0), tf


def _trainer(tmp_path, tag, prefetch=True, epochs=1, losses=None, enc=64, **kw):
    return P.Trainer(_network(enc), losses or [RecordRealInputs()], checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4,
                     epochs=epochs, recon=None, prefetch=prefetch, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(tr, loader, codes_of=None):
    del RECORDS[:]
    CODES_OF[0] = codes_of
    tr(loader)
    torch.cuda.synchronize()
    return list(RECORDS)


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("augment", ["none", "d4"])
def test_real_inputs_are_the_ref_of_the_tiles_in_the_loaders_order(tmp_path, prefetch, augment):
    tr = _trainer(tmp_path, "forms", prefetch, epochs=2)
    for form in ("tensor", "tuple", "dict"):
        loader, tf = _resident(form, augment)
        tr.start_epoch = 0
        got = _run(tr, loader, tf)
        assert len(got) == 2 * (TILES // BATCH) and loader.epoch == 2
        t = 0
        for e in range(2):
            order = epoch_order_ref(4, 0, e, TILES)
            for k in range(TILES // BATCH):
                image, codes, rna, labels = got[t]
                idx = order[k * BATCH:(k + 1) * BATCH]
                if augment == "d4":
                    assert np.array_equal(codes, tf.codes_for(t, BATCH)), (form, t)
                else:
                    assert codes is None
                assert np.array_equal(_bits(image), _bits(gather_transform_ref(_U8, idx, codes))), (form, t)
                if form != "tensor":
                    assert np.array_equal(labels, _LABELS[idx]), (form, t)          # the side data belongs to the image rows
                if form == "dict":
                    assert np.array_equal(_bits(rna), _bits(_RNA[_ROW_OF[idx]])), (form, t)
                t += 1
        assert tf.batches == (t if augment == "d4" else 0)


class _Replay(Sampler):
    """The resident loader's order of each epoch, batch by batch, for a host DataLoader."""

    def __init__(self, seed, epochs):
        self.seed, self.epoch, self.epochs = seed, 0, epochs

    def __len__(self):
        return TILES // BATCH

    def __iter__(self):
        order = epoch_order_ref(self.seed, 0, self.epoch, TILES)
        self.epoch += 1
        for k in range(TILES // BATCH):
            yield order[k * BATCH:(k + 1) * BATCH]


class _HostTiles(Dataset):
    def __len__(self):
        return TILES

    def __getitem__(self, i):
        return {"image": torch.from_numpy(_U8[i].copy()), "rna_data": torch.from_numpy(_RNA[_ROW_OF[i]].copy()),
                "labels": torch.tensor(_LABELS[i])}


@pytest.mark.parametrize("augment", ["none", "d4"])
def test_bit_identical_to_the_host_path_over_an_epoch(tmp_path, augment):
    loader, tf = _resident("dict", augment, seed=7)
    res = _run(_trainer(tmp_path, "res", epochs=2), loader, tf)
    host_tf = InputTransform(augment=augment, seed=7, rank=0)
    host = _run(_trainer(tmp_path, "host", epochs=2, input_transform=host_tf),
                DataLoader(_HostTiles(), batch_sampler=_Replay(7, 2)), host_tf)
    assert len(res) == len(host) == 2 * (TILES // BATCH)
    for t, ((a, ca, ra, la), (b, cb, rb, lb)) in enumerate(zip(res, host)):
        assert np.array_equal(_bits(a), _bits(b)), t
        assert (ca is None and cb is None) or np.array_equal(ca, cb), t
        assert np.array_equal(_bits(ra), _bits(rb)) and np.array_equal(la, lb), t


def test_resume_continues_order_and_codes(tmp_path):
    loader, tf = _resident("tuple", "d4", seed=9)
    whole = _run(_trainer(tmp_path, "whole", epochs=2), loader, tf)
    assert len(whole) == 6
    loader, tf = _resident("tuple", "d4", seed=9)
    _run(_trainer(tmp_path, "first", epochs=1), loader, tf)
    ck = torch.load(str(tmp_path / "ganfirst0.model"), map_location="cpu", weights_only=False)
    assert ck["data_loader"] == {"seed": 9, "epoch": 1, "transform": {"seed": 9, "augment": "d4", "batches": 3}}
    assert "input_transform" not in ck
    loader, tf = _resident("tuple", "d4", seed=9)
    second = _trainer(tmp_path, "second", epochs=2)
    second.load_model(load_path=str(tmp_path / "ganfirst0.model"))
    assert second.start_epoch == 1 and loader.epoch == 0 and tf.batches == 0          # applied by train()
    got = _run(second, loader, tf)
    assert len(got) == 3 and loader.epoch == 2 and tf.batches == 6
    for (a, ca, _, la), (b, cb, _, lb) in zip(whole[3:], got):
        assert np.array_equal(la, lb) and np.array_equal(ca, cb) and np.array_equal(_bits(a), _bits(b))
    assert any(not np.array_equal(la, lb) for (_, _, _, la), (_, _, _, lb) in zip(whole[:3], whole[3:]))   # a new order per epoch


def test_checkpoints_with_and_without_the_key(tmp_path):
    host = DataLoader(torch.from_numpy(gather_transform_ref(_U8[:12])), batch_size=BATCH)
    plain = _trainer(tmp_path, "plain")
    _run(plain, host)
    ck = torch.load(str(tmp_path / "ganplain0.model"), map_location="cpu", weights_only=False)
    assert "data_loader" not in ck                           # the checkpoint of a run without the feature is unchanged
    loader, tf = _resident("tensor", "d4", seed=2)
    with_res = _trainer(tmp_path, "with", epochs=2)
    with_res.load_model(load_path=str(tmp_path / "ganplain0.model"))          # no key: loads, the streams start at 0
    assert with_res.start_epoch == 1
    got = _run(with_res, loader, tf)
    assert len(got) == 3 and np.array_equal(got[0][1], tf.codes_for(0, BATCH))
    assert np.array_equal(_bits(got[0][0]), _bits(gather_transform_ref(_U8, epoch_order_ref(2, 0, 0, TILES)[:BATCH], got[0][1])))
    ck = torch.load(str(tmp_path / "ganwith0.model"), map_location="cpu", weights_only=False)
    assert ck["data_loader"]["epoch"] == 1 and ck["data_loader"]["transform"]["batches"] == 3
    other = _trainer(tmp_path, "other", epochs=3)
    other.load_model(load_path=str(tmp_path / "ganwith0.model"))             # the key is ignored by a plain DataLoader
    _run(other, host)
    assert "data_loader" not in torch.load(str(tmp_path / "ganother0.model"), map_location="cpu", weights_only=False)


def test_a_second_transform_is_refused(tmp_path):
    loader, _ = _resident("tuple", "d4")
    tr = _trainer(tmp_path, "twice", input_transform=InputTransform(augment="none"))
    with pytest.raises(ValueError, match="second time"):
        tr(loader)
    assert loader.epoch == 0


def test_real_wgan_iterations(tmp_path):
    """The stock plugins behind the resident loader: two iterations at batch 6 on the shapes tests/test_train_gpu.py trains in
    fp32 (out_size 16, 4 step channels, 2048 latent dimensions)."""
    torch.manual_seed(3)
    loader, tf = _resident("tuple", "d4", seed=6, batch=6)
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    tr = _trainer(tmp_path, "wgan", losses=losses, enc=2048, precision="fp32")
    tr(loader)
    torch.cuda.synchronize()
    assert tf.batches == 2
    for name in ("WassersteinGeneratorLoss", "WassersteinDiscriminatorLoss", "WassersteinGradientPenalty"):
        log = tr.loss_logs[name]
        assert len(log) == 2 and all(np.isfinite(v) for v in log), (name, log)
    assert tuple(tr.real_inputs.shape) == (6, 3, S, S) and tr.real_inputs.dtype == torch.float32
    want = gather_transform_ref(_U8, epoch_order_ref(6, 0, 0, TILES)[6:12], tf.last_codes)
    assert np.array_equal(_bits(tr.real_inputs.cpu().numpy()), _bits(want))
    for p in list(tr.generator.parameters()) + list(tr.discriminator.parameters()):
        assert torch.isfinite(p).all()


def test_cli_resident_and_d4(tmp_path):
    """The CLI end to end at 32 x 32 on synthetic tiles: the set built from the uint8 dataset, batches formed on the device, a
    per-epoch metric over the evaluation set's own path, and both streams' state in the checkpoint."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"path_csv": ["synthetic"], "patch_data_path": ["synthetic"], "img_size": 32, "rna_features": 16,
                               "save_dir": str(tmp_path), "flag": "resident"}))
    cmd = [sys.executable, os.path.join(repo, "histopathology_gan.py"), "--config", str(cfg), "--gan_type", "dcgan", "--loss_type", "wgan",
           "--synthetic", "--num_epochs", "2", "--steps_per_epoch", "3", "--resident", "1", "--resident_max_gb", "1", "--augment", "d4",
           "--kid_samples", "8", "--model_dir", str(tmp_path / "model"), "--image_dir", str(tmp_path / "img")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training of the Model is Complete" in r.stdout
    assert "Resident set on cuda:0: 24 tiles, %d bytes, 0 unreadable records dropped" % (24 * 3 * 32 * 32 + 24 * 4) in r.stdout
    ck = torch.load(str(tmp_path / "model1.model"), map_location="cpu", weights_only=False)
    assert ck["data_loader"] == {"seed": 99, "epoch": 2, "transform": {"seed": 99, "augment": "d4", "batches": 6}}
    assert "input_transform" not in ck
    assert all(len(v) == 6 and all(np.isfinite(x) for x in v) for v in ck["loss_logs"].values())
    kid = [float(line.split(":")[1]) for line in r.stdout.splitlines() if line.startswith("KernelDistance :")]
    assert len(kid) == 2 and all(np.isfinite(k) for k in kid)


def test_real_wganvae_iterations(tmp_path):
    """The VAE-conditioned plugins with a betaVAE over 64 RNA features (random weights) on the dict batches, two iterations at
    batch 6: the RNA rows come out of the de-duplicated table on the device."""
    torch.manual_seed(5)
    loader, tf = _resident("dict", "d4", seed=8, batch=6)
    kw = dict(checkpoint=None, rna_features=G)
    losses = [P.WassersteinGeneratorLossVAE(**kw), P.WassersteinDiscriminatorLossVAE(**kw), P.WassersteinGradientPenaltyVAE(**kw)]
    tr = _trainer(tmp_path, "vae", losses=losses, enc=2048, precision="fp32")
    tr(loader)
    torch.cuda.synchronize()
    assert tf.batches == 2
    for name in ("WassersteinGeneratorLossVAE", "WassersteinDiscriminatorLossVAE", "WassersteinGradientPenaltyVAE"):
        log = tr.loss_logs[name]
        assert len(log) == 2 and all(np.isfinite(v) for v in log), (name, log)
    idx = epoch_order_ref(8, 0, 0, TILES)[6:12]
    assert np.array_equal(_bits(tr.real_inputs["image"].cpu().numpy()), _bits(gather_transform_ref(_U8, idx, tf.last_codes)))
    assert np.array_equal(_bits(tr.real_inputs["rna_data"].cpu().numpy()), _bits(_RNA[_ROW_OF[idx]]))
    for p in list(tr.generator.parameters()) + list(tr.discriminator.parameters()):
        assert torch.isfinite(p).all()
