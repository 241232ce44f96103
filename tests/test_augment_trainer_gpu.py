"""Trainer(input_transform=...) on the GPU: what every loss plugin finds in ``real_inputs``.

A loss stub records the image of every batch (and the transform's codes at that moment); the yardstick is the numpy restatement
of tests/augment_refs.py applied to the loader's own uint8 tiles, bit for bit.  Networks: out_size 16, 4 step channels (nothing
of them runs under the stub); one test runs real ``wgan`` iterations on them."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import Adam
from torch.utils.data import DataLoader, Dataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from rna_gan_amd import losses as PL
from rna_gan_amd.augment import InputTransform
from augment_refs import normalize_ref, tile_transform_ref

S, BATCH, TILES = 16, 4, 12                 # three batches per epoch
RECORDS = []                                # (image as numpy, codes or None) per train_ops call of the stub


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
    """What a loss plugin sees: train_ops resolves ``real_inputs`` (and the trainer's transform) by name."""

    def train_ops(self, real_inputs, input_transform):
        image = real_inputs["image"] if isinstance(real_inputs, dict) else real_inputs
        # (a dict batch without a transform and without the prefetcher arrives on the host, as it always did: the plugins move it)
        assert image.dtype == torch.float32 and image.is_contiguous()
        assert image.is_cuda or input_transform is None
        codes = None if input_transform is None or input_transform.last_codes is None else input_transform.last_codes.copy()
        RECORDS.append((image.detach().cpu().numpy().copy(), codes))
        return 0.0


_U8 = np.random.default_rng(23).integers(0, 256, size=(TILES, 3, S, S), dtype=np.uint8)
_U8.setflags(write=False)


class _Tiles(Dataset):
    def __init__(self, form, as_u8):
        self.form = form
        self.x = torch.from_numpy(_U8.copy()) if as_u8 else torch.from_numpy(normalize_ref(_U8))
        self.rna = torch.from_numpy(np.random.default_rng(5).standard_normal((TILES, 6)).astype(np.float32))

    def __len__(self):
        return TILES

    def __getitem__(self, i):
        if self.form == "tensor":
            return self.x[i]
        if self.form == "tuple":
            return self.x[i], torch.tensor(0.0)
        return {"image": self.x[i], "rna_data": self.rna[i], "labels": torch.tensor(0.0)}


def _loader(form, as_u8):
    return DataLoader(_Tiles(form, as_u8), batch_size=BATCH)


def _trainer(tmp_path, tag, transform, prefetch=True, epochs=1, losses=None, enc=64, **kw):
    return P.Trainer(_network(enc), losses or [RecordRealInputs()], checkpoints=str(tmp_path / ("gan" + tag)), sample_size=4,
                     epochs=epochs, recon=None, prefetch=prefetch, input_transform=transform, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(tr, loader):
    del RECORDS[:]
    tr(loader)
    torch.cuda.synchronize()
    return list(RECORDS)


@pytest.mark.parametrize("prefetch", [True, False])
def test_none_on_uint8_is_the_float_loader_without_a_transform(tmp_path, prefetch):
    plain = _trainer(tmp_path, "plain", None, prefetch)
    tf = InputTransform(augment="none")
    dev = _trainer(tmp_path, "dev", tf, prefetch)
    for form in ("tuple", "tensor", "dict"):
        want = _run(plain, _loader(form, False))
        got = _run(dev, _loader(form, True))
        assert len(want) == len(got) == TILES // BATCH
        for k, ((a, _), (b, codes)) in enumerate(zip(want, got)):
            assert codes is None
            assert np.array_equal(_bits(a), _bits(b)), (form, k)
            assert np.array_equal(_bits(b), _bits(normalize_ref(_U8[k * BATCH:(k + 1) * BATCH]))), (form, k)
    assert tf.batches == 0 and tf.last_codes is None


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("as_u8", [True, False])
def test_d4_is_the_ref_transform_under_the_drawn_codes(tmp_path, prefetch, as_u8):
    tf = InputTransform(augment="d4", seed=4, rank=0)
    tr = _trainer(tmp_path, "d4", tf, prefetch)
    t = 0
    seen = set()
    for form in ("tuple", "tensor", "dict"):
        got = _run(tr, _loader(form, as_u8))
        assert len(got) == TILES // BATCH
        for k, (image, codes) in enumerate(got):
            assert np.array_equal(codes, tf.codes_for(t, BATCH)), (form, k)
            src = _U8[k * BATCH:(k + 1) * BATCH]
            want = tile_transform_ref(src if as_u8 else normalize_ref(src), codes)
            assert np.array_equal(_bits(image), _bits(want)), (form, k)
            seen.update(codes.tolist())
            t += 1
    assert tf.batches == t == 9
    assert len(seen) >= 4                                    # 36 draws: the batches were not all left as they were


def test_the_loaders_batch_objects_are_not_mutated(tmp_path):
    class Fixed:                                             # hands out the SAME objects on every pass
        batch_size = BATCH

        def __init__(self, batches):
            self.batches = batches

        def __iter__(self):
            return iter(self.batches)

        def __len__(self):
            return len(self.batches)

    u8 = [torch.from_numpy(_U8[k * BATCH:(k + 1) * BATCH].copy()) for k in range(TILES // BATCH)]
    labels = torch.zeros(BATCH)
    dicts = [{"image": x, "rna_data": torch.zeros(BATCH, 6), "labels": labels} for x in u8]
    lists = [[x, labels] for x in u8]
    tf = InputTransform(augment="d4", seed=1, rank=0)
    tr = _trainer(tmp_path, "fixed", tf, prefetch=False)
    for batches in (dicts, lists, list(u8)):
        got = _run(tr, Fixed(batches))
        for k, (image, codes) in enumerate(got):
            assert np.array_equal(_bits(image), _bits(tile_transform_ref(_U8[k * BATCH:(k + 1) * BATCH], codes)))
    for k, x in enumerate(u8):
        assert dicts[k]["image"] is x and lists[k][0] is x and sorted(dicts[k]) == ["image", "labels", "rna_data"]
        assert x.dtype == torch.uint8 and x.device.type == "cpu" and np.array_equal(x.numpy(), _U8[k * BATCH:(k + 1) * BATCH])


def test_resume_continues_the_code_stream(tmp_path):
    loader = _loader("tuple", True)
    whole = _run(_trainer(tmp_path, "whole", InputTransform(augment="d4", seed=9, rank=0), epochs=2), loader)
    assert len(whole) == 6
    first = _trainer(tmp_path, "first", InputTransform(augment="d4", seed=9, rank=0), epochs=1)
    _run(first, loader)
    ck = torch.load(str(tmp_path / "ganfirst0.model"), map_location="cpu", weights_only=False)
    assert ck["input_transform"] == {"seed": 9, "augment": "d4", "batches": 3}
    tf = InputTransform(augment="d4", seed=9, rank=0)
    second = _trainer(tmp_path, "second", tf, epochs=2)
    second.load_model(load_path=str(tmp_path / "ganfirst0.model"))
    assert second.start_epoch == 1 and tf.batches == 3
    got = _run(second, loader)
    assert len(got) == 3
    for (a, ca), (b, cb) in zip(whole[3:], got):
        assert np.array_equal(ca, cb) and np.array_equal(_bits(a), _bits(b))
    assert any(not np.array_equal(ca, cb) for (_, ca), (_, cb) in zip(whole[:3], whole[3:]))      # a new draw per batch


def test_checkpoints_with_and_without_the_key(tmp_path):
    loader = _loader("tuple", False)
    plain = _trainer(tmp_path, "plain", None)
    _run(plain, loader)
    ck = torch.load(str(tmp_path / "ganplain0.model"), map_location="cpu", weights_only=False)
    assert "input_transform" not in ck                       # the checkpoint of a run without the feature is unchanged
    tf = InputTransform(augment="d4", seed=2, rank=0)
    with_tf = _trainer(tmp_path, "with", tf, epochs=2)
    with_tf.load_model(load_path=str(tmp_path / "ganplain0.model"))          # no key: loads, the stream starts at 0
    assert with_tf.start_epoch == 1 and tf.batches == 0
    got = _run(with_tf, loader)
    assert np.array_equal(got[0][1], tf.codes_for(0, BATCH))
    ck = torch.load(str(tmp_path / "ganwith0.model"), map_location="cpu", weights_only=False)
    assert ck["input_transform"]["batches"] == 3
    other = _trainer(tmp_path, "other", None, epochs=2)
    other.load_model(load_path=str(tmp_path / "ganwith0.model"))             # the key is ignored without a transform
    assert other.start_epoch == 2 and other.input_transform is None


def test_real_wgan_iterations_with_d4(tmp_path):
    """The stock plugins behind the transform: two iterations at batch 6 on the shapes tests/test_train_gpu.py trains in fp32
    (out_size 16, 4 step channels, 2048 latent dimensions)."""
    torch.manual_seed(3)
    tf = InputTransform(augment="d4", seed=6, rank=0)
    losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    tr = _trainer(tmp_path, "wgan", tf, losses=losses, enc=2048, precision="fp32")
    tr(DataLoader(_Tiles("tuple", True), batch_size=6))
    torch.cuda.synchronize()
    assert tf.batches == 2
    for name in ("WassersteinGeneratorLoss", "WassersteinDiscriminatorLoss", "WassersteinGradientPenalty"):
        log = tr.loss_logs[name]
        assert len(log) == 2 and all(np.isfinite(v) for v in log), (name, log)
    assert tuple(tr.real_inputs.shape) == (6, 3, S, S) and tr.real_inputs.dtype == torch.float32
    want = tile_transform_ref(_U8[6:], tf.last_codes)
    assert np.array_equal(_bits(tr.real_inputs.cpu().numpy()), _bits(want))
    for p in list(tr.generator.parameters()) + list(tr.discriminator.parameters()):
        assert torch.isfinite(p).all()


def test_cli_device_transform_and_d4(tmp_path):
    """The CLI end to end at 32 x 32 on synthetic tiles: uint8 from the loader, normalised and augmented on the device, a per-epoch
    metric over the unaugmented set, and the code stream's counter in the checkpoint."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"path_csv": ["synthetic"], "patch_data_path": ["synthetic"], "img_size": 32, "rna_features": 16,
                               "save_dir": str(tmp_path), "flag": "augment"}))
    cmd = [sys.executable, os.path.join(repo, "histopathology_gan.py"), "--config", str(cfg), "--gan_type", "dcgan", "--loss_type", "wgan",
           "--synthetic", "--num_epochs", "1", "--steps_per_epoch", "3", "--device_transform", "1", "--augment", "d4",
           "--kid_samples", "8", "--model_dir", str(tmp_path / "model"), "--image_dir", str(tmp_path / "img")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training of the Model is Complete" in r.stdout
    ck = torch.load(str(tmp_path / "model0.model"), map_location="cpu", weights_only=False)
    assert ck["input_transform"] == {"seed": 99, "augment": "d4", "batches": 3}
    assert all(len(v) == 3 and all(np.isfinite(x) for x in v) for v in ck["loss_logs"].values())
    # (an epoch's checkpoint is written before its evaluation: the metric's value is on the console)
    kid = [float(line.split(":")[1]) for line in r.stdout.splitlines() if line.startswith("KernelDistance :")]
    assert len(kid) == 1 and np.isfinite(kid[0])
