"""The resident expression table in front of the betaVAE training loop, and the three CLIs, on the device: a small model
(``encoder_dims`` / ``decoder_dims``), F = 130 genes, two tables of 40 + 30 rows, batch 8.

(i)   what train_betaVAE receives from RnaTableLoader is the table's rows in the epoch order;
(ii)  three training iterations over the resident loader give bit-identical losses and parameters to the same iterations over
      a host DataLoader that replays the same order, and the resident loader consumes no torch random numbers;
(iii) betaVAE_training.py end to end on two CSV files; --resident 0 gives the same split and scaler;
(iv)  betaVAE_interpolation.py --type tissue, then betaVAE_sample.py --interpolation, on that checkpoint;
(v)   --synthetic still runs."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

import rna_gan_amd as P
from rna_gan_amd import rna_tables as RT
from rna_gan_amd import vae_train as VT
from oracle import ref_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, ROWS, BATCH, SEED = 130, (40, 30), 8, 99
ENC, DEC = [96, 64, 32], [64, 96]
_CACHE = {}


def _frames():
    if "frames" not in _CACHE:
        rng = np.random.default_rng(61)
        frames = []
        for t, m in enumerate(ROWS):
            rna = np.round(rng.gamma(1.5, 20.0, size=(m, F)) * (1.0 + 0.5 * t), 3)
            rna[rng.integers(0, m, size=20), rng.integers(0, F, size=20)] = 0.0
            cols = {"wsi_file_name": ["GTEX-T%d-%04d.svs" % (t, i) for i in range(m)]}
            cols.update({"rna_G%d" % j: rna[:, j] for j in range(F)})
            frames.append(pd.DataFrame(cols))
        _CACHE["frames"] = frames
        _CACHE["prepared"] = RT.prepare_tables(frames, SEED)
    return _CACHE["frames"], _CACHE["prepared"]


def _cli(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(seed=71):
    m = P.betaVAE(F, ENC[-1], ENC, DEC, beta=0.5)
    R.seeded_fill_(m, seed)
    return m.set_precision("bf16").cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


class _Recording:
    """A loader that keeps a copy of every batch it hands on."""

    def __init__(self, loader):
        self.loader, self.seen = loader, []

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            self.seen.append(b["rna_data"].clone())
            yield b


def _table():
    _frames_, (rows, _scaler, _indices, _parts) = _frames()
    all_rows = np.concatenate([rows[k] for k in RT.PARTS], axis=0)
    n_train, n_val = rows["train"].shape[0], rows["val"].shape[0]
    assert (n_train, n_val, rows["test"].shape[0]) == (44, 12, 14) and all_rows.shape == (70, F)
    return all_rows, n_train, n_val


def _train(loaders, epochs, tmp_path, name):
    torch.manual_seed(5)
    m = _model()
    opt = P.Adam(m.parameters(), lr=2e-3, weight_decay=1e-5).bind(m)
    m, res = VT.train_betaVAE(m, opt, loaders, save_dir=str(tmp_path / name), num_epochs=epochs, verbose=False)
    return torch.load(str(tmp_path / name / "model_last.pt"), map_location="cpu"), res


def test_train_loop_receives_the_epoch_order(tmp_path):
    all_rows, n_train, n_val = _table()
    ts = RT.RnaTableSet.from_array(all_rows, "cuda:0")
    assert ts.device.type == "cuda" and ts.nbytes == 70 * F * 4
    train = _Recording(RT.RnaTableLoader(ts, np.arange(n_train), BATCH, shuffle=True, seed=SEED, drop_last=True))
    val = _Recording(RT.RnaTableLoader(ts, np.arange(n_train, n_train + n_val), BATCH))
    _train({"train": train, "val": val}, 2, tmp_path, "a")
    assert len(train.seen) == 2 * 5 and len(val.seen) == 2 * 2 and train.loader.epoch == 2 and val.loader.epoch == 2
    for e in range(2):
        order = np.random.default_rng([SEED, 0, e]).permutation(n_train)
        for t in range(5):
            x = train.seen[5 * e + t]
            assert x.device.type == "cuda" and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (BATCH, F)
            assert np.array_equal(x.cpu().numpy().view(np.uint32), all_rows[order[t * BATCH:(t + 1) * BATCH]].view(np.uint32))
        assert np.array_equal(val.seen[2 * e].cpu().numpy().view(np.uint32), all_rows[n_train:n_train + 8].view(np.uint32))
        assert np.array_equal(val.seen[2 * e + 1].cpu().numpy().view(np.uint32), all_rows[n_train + 8:n_train + 12].view(np.uint32))
    # _to_device has nothing left to do: the batch it returns is the loader's tensor
    b = next(iter(RT.RnaTableLoader(ts, np.arange(8), BATCH)))
    assert VT._to_device(b, ts.device) is b["rna_data"]


def test_resident_loader_equals_a_host_loader_replaying_its_order(tmp_path):
    all_rows, _n_train, n_val = _table()
    items = np.arange(3, 27)                                        # 24 rows: three iterations
    val_items = np.arange(44, 44 + n_val)
    ts = RT.RnaTableSet.from_array(all_rows, "cuda:0")
    res_train = RT.RnaTableLoader(ts, items, BATCH, shuffle=True, seed=SEED, drop_last=True)
    # the loader consumes no torch random numbers, on either generator
    torch.manual_seed(3)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    order = [b["rna_data"] for b in res_train]
    assert len(order) == 3
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
    res_train.load_state_dict({"seed": SEED, "epoch": 0})
    sd_a, res_a = _train({"train": res_train, "val": RT.RnaTableLoader(ts, val_items, BATCH)}, 1, tmp_path, "res")
    host = RT.RNADataset([all_rows])
    replay = RT.epoch_order(SEED, 0, items).tolist()
    batches = [replay[t * BATCH:(t + 1) * BATCH] for t in range(3)]
    loaders = {"train": torch.utils.data.DataLoader(host, batch_sampler=batches),
               "val": torch.utils.data.DataLoader(host, batch_sampler=[val_items[:8].tolist(), val_items[8:].tolist()])}
    sd_b, res_b = _train(loaders, 1, tmp_path, "host")
    assert res_a["history"] == res_b["history"], (res_a["history"], res_b["history"])
    assert np.isfinite(res_a["history"]["train"]["total_loss"]).all()
    assert sorted(sd_a) == sorted(sd_b)
    for k in sd_a:
        assert torch.equal(_bits(sd_a[k]), _bits(sd_b[k])), k


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One real-table training run of the CLI (one epoch) shared by the CLI tests."""
    d = tmp_path_factory.mktemp("vae_cli")
    frames, _ = _frames()
    paths = []
    for i, df in enumerate(frames):
        paths.append(str(d / ("tissue%d.csv" % i)))
        df.to_csv(paths[-1], index=False)
    config = {"save_dir": str(d / "out"), "path_csv": paths, "rna_features": F, "batch_size": BATCH, "beta": 0.5, "lr": 1e-3,
              "weights_decay": 1e-5, "num_epochs": 1, "log_interval": 100, "warmup_steps": 2, "encoder_dims": ENC,
              "decoder_dims": DEC, "num_workers": 0}
    cfg = str(d / "config.json")
    with open(cfg, "w") as f:
        json.dump(config, f)
    _cli("betaVAE_training").main(["--config", cfg, "--seed", str(SEED)])
    return {"dir": d, "config": config, "cfg": cfg}


def test_training_cli_end_to_end(run):
    out = run["config"]["save_dir"]
    for name in ("model_last.pt", "model_dict_best.pt", "scaler.npz", "split.npz", "test_results.pkl"):
        assert os.path.exists(os.path.join(out, name)), name
    _frames_, (rows, scaler, indices, _parts) = _frames()
    saved = RT.RnaScaler.load(os.path.join(out, "scaler.npz"))
    assert np.array_equal(saved.mean.view(np.uint64), scaler.mean.view(np.uint64))
    assert np.array_equal(saved.scale.view(np.uint64), scaler.scale.view(np.uint64)) and saved.columns == scaler.columns
    with np.load(os.path.join(out, "split.npz")) as s:
        for i in (0, 1):
            for k in RT.PARTS:
                assert s["%s_%d" % (k, i)].tolist() == indices[i][k].tolist()
    sd = torch.load(os.path.join(out, "model_last.pt"), map_location="cpu")
    assert tuple(sd["encoder.encoder.1.0.weight"].shape) == (ENC[0], F) and all(torch.isfinite(v).all() for v in sd.values())
    with open(os.path.join(out, "test_results.pkl"), "rb") as f:
        res = pickle.load(f)
    assert res["predictions"].shape == (14, F) and res["test_labels"].tolist() == [0] * 8 + [1] * 6
    assert np.array_equal(res["real"].view(np.uint32), scaler.inverse_transform(rows["test"]).view(np.uint32))
    # the reference's route under the same seed: the same split and scaler
    config = dict(run["config"], save_dir=str(run["dir"] / "out_host"))
    cfg = str(run["dir"] / "config_host.json")
    with open(cfg, "w") as f:
        json.dump(config, f)
    _cli("betaVAE_training").main(["--config", cfg, "--seed", str(SEED), "--resident", "0"])
    assert os.path.exists(os.path.join(config["save_dir"], "model_last.pt"))
    host = RT.RnaScaler.load(os.path.join(config["save_dir"], "scaler.npz"))
    assert np.array_equal(host.mean.view(np.uint64), saved.mean.view(np.uint64))
    assert np.array_equal(host.scale.view(np.uint64), saved.scale.view(np.uint64))
    with np.load(os.path.join(out, "split.npz")) as a, np.load(os.path.join(config["save_dir"], "split.npz")) as b:
        assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)


def test_interpolation_then_sample(run):
    out = run["config"]["save_dir"]
    ckpt = os.path.join(out, "model_last.pt")
    _cli("betaVAE_interpolation").main(["--config", run["cfg"], "--checkpoint", ckpt, "--seed", str(SEED), "--type", "tissue"])
    with open(os.path.join(out, "interpolation_lung_sex_results.pkl"), "rb") as f:
        res = pickle.load(f)
    assert sorted(res) == sorted(["z_mu1", "z_mu2", "z_logvar1", "z_logvar2", "sample1_encod", "sample2_encod", "sample1", "sample2",
                                  "recons_1", "recons_2", "z_a_to_b", "z_b_to_a"])
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 and np.isfinite(v).all() for v in res.values())
    Z = ENC[-1]
    n = (25, 19)                                                    # the train rows of the two tables
    for g in (1, 2):
        assert res["z_mu%d" % g].shape == res["z_logvar%d" % g].shape == res["sample%d_encod" % g].shape == (n[g - 1], Z)
        assert res["sample%d" % g].shape == res["recons_%d" % g].shape == (n[g - 1], F)
    assert res["z_a_to_b"].shape == (Z,) and np.array_equal(res["z_a_to_b"], -res["z_b_to_a"])
    c1, c2 = res["z_mu1"].astype(np.float64).mean(axis=0), res["z_mu2"].astype(np.float64).mean(axis=0)
    assert np.array_equal(res["z_a_to_b"], (c1 - c2).astype(np.float32)) and np.abs(res["z_a_to_b"]).max() > 0
    # the groups are the standardised train rows of each table, in split order
    frames, (_rows, scaler, indices, _parts) = _frames()
    for g in (0, 1):
        want = scaler.transform_frame(frames[g].iloc[indices[g]["train"]]).astype(np.float32)
        assert np.array_equal(res["sample%d" % (g + 1)].view(np.uint32), want.view(np.uint32))
    # the same model recomputes what the file holds
    model = RT.model_from_config(run["config"], F)
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    model = model.set_precision("bf16").cuda().eval()
    with torch.no_grad():
        mu, _lv, enc = model.encode(torch.from_numpy(res["sample1"]).cuda())
        rec = model.decode(enc + torch.from_numpy(res["z_a_to_b"]).cuda())
    assert torch.equal(mu.cpu(), torch.from_numpy(res["z_mu1"])) and torch.equal(rec.cpu(), torch.from_numpy(res["recons_1"]))
    # the two groups by a column of the first table: the same code path with other rows
    merged = str(run["dir"] / "merged.csv")
    df = frames[0].copy()
    df["SEX"] = [1 + (i % 2) for i in range(df.shape[0])]
    df.to_csv(merged, index=False)
    config = dict(run["config"], path_csv=[merged])
    cfg = str(run["dir"] / "config_sex.json")
    with open(cfg, "w") as f:
        json.dump(config, f)
    by_sex = str(run["dir"] / "by_sex.pkl")
    _cli("betaVAE_interpolation").main(["--config", cfg, "--checkpoint", ckpt, "--seed", str(SEED), "--group_column", "SEX",
                                        "--group_a", "1", "--group_b", "2", "--scaler", os.path.join(out, "scaler.npz"),
                                        "--out", by_sex])
    with open(by_sex, "rb") as f:
        sex = pickle.load(f)
    assert sex["sample1"].shape[0] + sex["sample2"].shape[0] == 25 and np.array_equal(sex["z_a_to_b"], -sex["z_b_to_a"])

    # ---- betaVAE_sample.py --interpolation on that file
    _cli("betaVAE_sample").main(["--config", run["cfg"], "--checkpoint", ckpt, "--seed", "7", "--num_samples", "6",
                                 "--interpolation", os.path.join(out, "interpolation_lung_sex_results.pkl"), "--alpha", "0.5"])
    with open(os.path.join(out, "generated_samples_interpolation_lung.pkl"), "rb") as f:
        gen = pickle.load(f)
    assert sorted(gen) == ["generated"] and gen["generated"].shape == (6, F) and gen["generated"].dtype == np.float32
    # the program seeds first and builds the model next, as the reference does: the latents follow the initialisation's draws
    torch.manual_seed(7)
    RT.model_from_config(run["config"], F)
    z = torch.randn(6, Z) + torch.from_numpy(0.5 * res["z_b_to_a"]).float()
    with torch.no_grad():
        decoded = model.decode(z.cuda()).cpu().numpy()
    assert np.array_equal(gen["generated"].view(np.uint32), scaler.inverse_transform(decoded).view(np.uint32))
    # no scaler file anywhere: refitted by repeating the split under the seed
    config = dict(run["config"], save_dir=str(run["dir"] / "elsewhere"))
    cfg = str(run["dir"] / "config_elsewhere.json")
    with open(cfg, "w") as f:
        json.dump(config, f)
    _cli("betaVAE_sample").main(["--config", cfg, "--checkpoint", ckpt, "--seed", str(SEED), "--num_samples", "3"])
    with open(os.path.join(config["save_dir"], "generated_samples_interpolation_lung.pkl"), "rb") as f:
        plain = pickle.load(f)
    torch.manual_seed(SEED)
    RT.model_from_config(run["config"], F)
    with torch.no_grad():
        decoded = model.decode(torch.randn(3, Z).cuda()).cpu().numpy()
    assert np.array_equal(plain["generated"].view(np.uint32), scaler.inverse_transform(decoded).view(np.uint32))


def test_synthetic_path_still_runs(tmp_path):
    config = {"save_dir": str(tmp_path / "syn"), "rna_features": 64, "batch_size": 16, "num_epochs": 1, "warmup_steps": 2}
    cfg = str(tmp_path / "c.json")
    with open(cfg, "w") as f:
        json.dump(config, f)
    _cli("betaVAE_training").main(["--config", cfg, "--synthetic", "--samples", "32"])
    out = config["save_dir"]
    assert os.path.exists(os.path.join(out, "model_last.pt")) and not os.path.exists(os.path.join(out, "scaler.npz"))
    sd = torch.load(os.path.join(out, "model_last.pt"), map_location="cpu")
    assert tuple(sd["encoder.encoder.1.0.weight"].shape) == (6000, 64)
