#!/usr/bin/env python3
"""Working counterpart of the reference's src/betaVAE_training.py on the MI355X path.

Same flags (--config --checkpoint --seed --log --parallel) and JSON keys (save_dir, rna_features, batch_size, beta,
optimizer, lr, weights_decay, num_epochs, log_interval); model / optimizer / scheduler construction follows
src/betaVAE_training.py:131-176 (betaVAE(rna_features, 2048, [6000, 4000, 2048], [4000, 6000], beta), xavier init,
Adam(weight_decay, lr), CosineAnnealingLR(500)); the loop is rna_gan_amd.vae_train.train_betaVAE.

Real tables (the default): the config's ``path_csv`` (a list of CSV files, one per tissue), ``quick`` and ``rna_features`` are
the reference's.  The sequence is src/betaVAE_training.py:60-112 -- ``np.random.seed(seed)``, pandas ``read_csv``, the 80/20 +
80/20 split per table, ln + StandardScaler fitted on the train split (rna_gan_amd.rna_tables) -- after which the standardised
rows of all three splits live on the device as ONE fp32 table and every batch is formed there by one launch
(``RnaTableSet`` / ``RnaTableLoader``, rg_rows_gather_f32): no DataLoader workers, no collate, no per-batch host-to-device copy.
``--resident 0`` trains over ``DataLoader(RNADataset)`` instead, the reference's route.  ``scaler.npz`` (mean, scale, column
names), ``split.npz`` (the three index lists per CSV, ``train_0`` / ``val_0`` / ``test_0`` ...) and, as the reference does,
``test_results.pkl`` are written into ``save_dir``; betaVAE_sample.py and betaVAE_interpolation.py read the first.
Optional config keys ``encoder_dims`` / ``decoder_dims`` default to the reference's [6000, 4000, 2048] / [4000, 6000].

Deviation: the train loader shuffles with ``drop_last=True`` -- train-mode BatchNorm1d cannot take a last batch of one row --
where the reference keeps the partial batch; val and test are sequential and keep theirs (test in batches of ``batch_size``,
the reference's batch of 1 computes the same rows in eval mode).

``--synthetic`` trains on standardised synthetic expression rows of the right width, with no table at all.  The
reference's GradualWarmupScheduler (third-party ``warmup_scheduler``, absent here) is replaced by torch's LinearLR
warm-up chained in front of the same cosine schedule.
"""
import argparse
import json
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

import rna_gan_amd as P
from rna_gan_amd import rna_tables as RT
from rna_gan_amd import vae_train as VT


class SyntheticRNA(Dataset):
    """N(0,1) rows squashed into tanh's range (StandardScaler output; the decoder ends in Tanh)."""

    def __init__(self, n, features, seed):
        rng = np.random.default_rng(seed)
        self.rows = torch.from_numpy(np.tanh(rng.normal(size=(n, features)).astype(np.float32)))

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, i):
        return {"rna_data": self.rows[i]}


def init_weights_xavier(m):
    if isinstance(m, torch.nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight)
        m.bias.data.fill_(0.01)


def real_tables(args, config):
    """The reference's sequence up to the datasets (host, fp64, once): seed, read, split, fit on train, transform all three.
    Everything here runs before the device is touched, so a bad config is reported without one."""
    if not config.get("path_csv"):
        raise SystemExit("betaVAE_training: the config has no 'path_csv' (the list of RNA-Seq CSV files, one per tissue); "
                         "give it, or train on synthetic rows with --synthetic")
    np.random.seed(args.seed)
    frames = RT.read_tables(config)
    rows, scaler, indices, parts = RT.prepare_tables(frames, args.seed)
    features = RT.check_features(config, rows["train"].shape[1])
    for k in RT.PARTS:
        print("{} shape {}".format(k.capitalize(), parts[k].shape))
    train_items = np.arange(rows["train"].shape[0])
    if config.get("quick", 0):
        # the reference's RNADataset(quick=True): DataFrame.sample(10) of the train frame on numpy's global generator
        train_items = np.sort(parts["train"].reset_index(drop=True).sample(10).index.to_numpy())
    os.makedirs(config["save_dir"], exist_ok=True)
    scaler.save(os.path.join(config["save_dir"], "scaler.npz"))
    np.savez(os.path.join(config["save_dir"], "split.npz"),
             **{"%s_%d" % (k, i): np.asarray(idx[k], dtype=np.int64) for i, idx in enumerate(indices) for k in RT.PARTS})
    test_labels = np.concatenate([np.full(len(idx["test"]), i, dtype=np.int64) for i, idx in enumerate(indices)])
    return {"rows": rows, "scaler": scaler, "features": features, "train_items": train_items,
            "test_ids": parts["test"]["wsi_file_name"].values if "wsi_file_name" in parts["test"].columns else None,
            "test_labels": test_labels}


def real_loaders(args, config, tables, batch_size):
    rows = tables["rows"]
    if batch_size > len(tables["train_items"]):
        raise SystemExit("batch_size %d exceeds the %d train rows (the train loader drops the partial batch)"
                         % (batch_size, len(tables["train_items"])))
    if not args.resident:
        return {"train": DataLoader(RT.RNADataset([rows["train"][tables["train_items"]]]), batch_size=batch_size, shuffle=True,
                                    drop_last=True, num_workers=config.get("num_workers", 4)),
                "val": DataLoader(RT.RNADataset([rows["val"]]), batch_size=batch_size),
                "test": DataLoader(RT.RNADataset([rows["test"]]), batch_size=batch_size)}
    n_train, n_val, n_test = (rows[k].shape[0] for k in RT.PARTS)
    table = RT.RnaTableSet.from_array(np.concatenate([rows[k] for k in RT.PARTS], axis=0), "cuda:0")
    return {"train": RT.RnaTableLoader(table, tables["train_items"], batch_size, shuffle=True, seed=args.seed, drop_last=True),
            "val": RT.RnaTableLoader(table, np.arange(n_train, n_train + n_val), batch_size),
            "test": RT.RnaTableLoader(table, np.arange(n_train + n_val, n_train + n_val + n_test), batch_size)}


def evaluate_real(model, test_loader, tables, save_dir):
    """evaluate_betaVAE on the test split and the reference's test_results.pkl (src/betaVAE_training.py:190-202)."""
    import pickle
    test_loss, predictions, real = VT.evaluate_betaVAE(model, test_loader)
    scaler = tables["scaler"]
    results = {"predictions": scaler.inverse_transform(np.vstack(predictions).astype(np.float32)),
               "real": scaler.inverse_transform(np.vstack(real).astype(np.float32)),
               "test_ids": tables["test_ids"], "test_labels": tables["test_labels"]}
    with open(os.path.join(save_dir, "test_results.pkl"), "wb") as f:
        pickle.dump(results, f)
    return test_loss


def main(argv=None):
    ap = argparse.ArgumentParser(description="betaVAE training over RNA-Seq data (MI355X path)")
    ap.add_argument("--config", type=str, help="JSON config file")
    ap.add_argument("--checkpoint", type=str, default=None, help="File with the checkpoint to start with")
    ap.add_argument("--seed", type=int, default=99, help="Seed for random generation")
    ap.add_argument("--log", type=int, default=0, help="Use tensorboard for experiment logging (needs tensorboardX)")
    ap.add_argument("--parallel", type=int, default=None, help="accepted for compatibility; one process drives one GPU")
    ap.add_argument("--synthetic", action="store_true", help="train on synthetic standardised expression rows")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--samples", type=int, default=1024, help="synthetic training rows")
    ap.add_argument("--resident", type=int, default=1,
                    help="real tables: 1 = the table on the device, one launch per batch; 0 = DataLoader(RNADataset)")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    print(10 * "-"); print("Config for this experiment \n"); print(config); print(10 * "-")
    tables = None if args.synthetic else real_tables(args, config)
    torch.manual_seed(args.seed)
    batch_size = config.get("batch_size", 64)
    os.makedirs(config["save_dir"], exist_ok=True)
    if tables is None:
        rna_features = config.get("rna_features", 19198)
        loaders = {"train": DataLoader(SyntheticRNA(args.samples, rna_features, args.seed), batch_size=batch_size, shuffle=True,
                                       drop_last=True),
                   "val": DataLoader(SyntheticRNA(max(batch_size, args.samples // 8), rna_features, args.seed + 1),
                                     batch_size=batch_size)}
        model = P.betaVAE(rna_features, 2048, [6000, 4000, 2048], [4000, 6000], beta=config.get("beta", 2))
    else:
        loaders = real_loaders(args, config, tables, batch_size)
        model = RT.model_from_config(config, tables["features"])
    if args.checkpoint is not None:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    else:
        model.apply(init_weights_xavier)
    model = model.set_precision(args.precision).cuda()
    if config.get("optimizer", "Adam") != "Adam":
        raise SystemExit("only Adam has a fused HIP step (the reference's default)")
    optimizer = P.Adam(model.parameters(), weight_decay=config.get("weights_decay", 0.0), lr=config.get("lr", 3e-3)).bind(model)
    cosine = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, 500)
    warm = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=1e-3, total_iters=config.get("warmup_steps", 1000))
    scheduler = torch.optim.lr_scheduler.SequentialLR(optimizer, [warm, cosine], milestones=[config.get("warmup_steps", 1000)])
    writer = None
    if args.log:
        from tensorboardX import SummaryWriter
        writer = SummaryWriter(config.get("summary_path", os.path.join(config["save_dir"], "tb")))
    model, results = VT.train_betaVAE(model, optimizer, loaders, save_dir=config["save_dir"],
                                      log_interval=config.get("log_interval", 100), summary_writer=writer,
                                      num_epochs=config.get("num_epochs", 5), scheduler=scheduler)
    if tables is not None:
        test_loss = evaluate_real(model, loaders["test"], tables, config["save_dir"])
    else:
        test_loss, _, _ = VT.evaluate_betaVAE(model, loaders["val"])
    print("best epoch", results["best_epoch"], "best validation loss", results["best_loss"], "final", test_loss)


if __name__ == "__main__":
    main()
