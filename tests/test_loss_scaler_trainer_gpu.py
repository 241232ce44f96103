"""Dynamic loss scaling through the public interface: the CLI (`--precision fp16 --loss_scaling dynamic`) on the mixed-tissue
tables, and a Trainer checkpoint round trip that restores the scale and the growth tracker."""
import os
import subprocess

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from oracle import ref_cpu as R
from test_trainer_gpu import network, _mixed_tissue_config, _cli_cmd, _checkpoint_files


def test_cli_fp16_dynamic_loss_scaling_on_mixed_tissue_tables(tmp_path):
    cfg_path = _mixed_tissue_config(tmp_path)
    r = subprocess.run(_cli_cmd(tmp_path, cfg_path) + ["--precision", "fp16", "--loss_scaling", "dynamic"], capture_output=True,
                       text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training of the Model is Complete" in r.stdout
    vals = [float(l.split(":")[1]) for l in r.stdout.splitlines() if "Mean Loss" in l]
    assert len(vals) >= 2 and all(np.isfinite(v) for v in vals)
    assert any(l.startswith("loss scale :") for l in r.stdout.splitlines())         # the epoch line reports the scaler
    files = _checkpoint_files(tmp_path)
    assert files, "no checkpoint written"
    ck = torch.load(files[0], map_location="cpu", weights_only=False)
    sc = ck["loss_scaler"]
    assert set(sc) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker", "skipped_steps"}
    assert sc["growth_interval"] == 2000 and sc["scale"] >= 1.0
    # the optimizers report the steps their device counters took (skipped steps do not count)
    g_steps = int(float(ck["optimizer_generator"]["state"][0]["step"]))
    d_steps = int(float(ck["optimizer_discriminator"]["state"][0]["step"]))
    iters = ck["loss_information"]["generator_iters"]
    assert g_steps + d_steps == 3 * iters - sc["skipped_steps"]
    for net in ("generator", "discriminator"):
        for k, v in ck[net].items():
            assert not v.dtype.is_floating_point or bool(torch.isfinite(v).all()), (net, k)


def test_trainer_checkpoint_restores_scale_and_tracker(tmp_path):
    torch.manual_seed(0)
    imgs = R.synthetic_images(32, 32, seed=5)
    loader = DataLoader(TensorDataset(imgs, torch.zeros(32)), batch_size=8)       # 4 iterations = 12 train_ops
    losses = lambda: [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
    ck = str(tmp_path / "gan")
    tr = P.Trainer(network(), losses(), checkpoints=ck, sample_size=4, epochs=1, recon=str(tmp_path / "img"), nrow=2,
                   loss_scaling="dynamic", loss_scaling_args={"init_scale": 2.0 ** 10, "growth_interval": 5})
    tr(loader)
    assert tr.loss_scaler.get_scale() == 2.0 ** 12                                # 12 clean train_ops: two growths
    sd = torch.load(ck + "0.model", map_location="cpu", weights_only=False)
    assert sd["loss_scaler"]["scale"] == 2.0 ** 12 and sd["loss_scaler"]["_growth_tracker"] == 2
    tr2 = P.Trainer(network(), losses(), checkpoints=str(tmp_path / "gan2"), sample_size=4, epochs=1,
                    recon=str(tmp_path / "img2"), loss_scaling="dynamic")
    assert tr2.loss_scaler.get_scale() == 4096.0
    tr2.load_model(load_path=ck + "0.model")
    got = tr2.loss_scaler.state_dict()
    assert got["scale"] == 2.0 ** 12 and got["_growth_tracker"] == 2 and got["growth_interval"] == 5
    # a trainer without a scaler loads the checkpoint unchanged and keeps writing today's keys
    tr3 = P.Trainer(network(), losses(), checkpoints=str(tmp_path / "gan3"), sample_size=4, epochs=1,
                    recon=str(tmp_path / "img3"))
    assert tr3.loss_scaler is None
    tr3.load_model(load_path=ck + "0.model")
    tr3.save_model(0)
    assert "loss_scaler" not in torch.load(str(tmp_path / "gan3") + "0.model", map_location="cpu", weights_only=False)
