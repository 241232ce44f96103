#!/usr/bin/env python3
"""Working counterpart of the reference's src/betaVAE_interpolation.py on the MI355X path: latent arithmetic between two cohorts.

``--type tissue`` takes the train rows of the first two CSVs of the config's ``path_csv``; ``--group_column COL --group_a A
--group_b B`` takes the train rows of the FIRST table whose column COL equals A / B (the reference's ``sex`` case once the
phenotype column has been merged into the table; its hard-coded GTEx annotation path is not reproduced).  The split is the
training run's (the same seed), the rows of each group are standardised with the shared scaler (``--scaler``, else
``scaler.npz`` in ``save_dir``, else refitted from the split), ``model.encode`` runs in eval mode on the HIP kernels in chunks,
the centroids of ``z_mu`` are fp64 column means taken on the host, and each group's encodings are decoded after moving them by
the difference of the centroids.

Output: the reference's pickle (its file name, in ``save_dir``, unless --out is given) with its keys, all numpy arrays:
z_mu1/2, z_logvar1/2, sample1/2_encod, sample1/2, recons_1/2, z_a_to_b (= centroid 1 - centroid 2), z_b_to_a.
betaVAE_sample.py --interpolation reads it.  The reference's ``tissue`` branch ends in a NameError, because it stores
``male_df`` / ``female_df``, which only the ``sex`` branch defines; this one stores the two groups' rows in either case.
"""
import argparse
import json
import os
import pickle

import numpy as np
import torch

from rna_gan_amd import rna_tables as RT


def encode_chunks(model, rows, chunk):
    mu, lv, enc = [], [], []
    with torch.no_grad():
        for i in range(0, rows.shape[0], chunk):
            m, v, e = model.encode(torch.from_numpy(rows[i:i + chunk]).cuda())
            mu.append(m.cpu().numpy()); lv.append(v.cpu().numpy()); enc.append(e.cpu().numpy())
    return np.concatenate(mu), np.concatenate(lv), np.concatenate(enc)


def decode_chunks(model, z, chunk):
    out = []
    with torch.no_grad():
        for i in range(0, z.shape[0], chunk):
            out.append(model.decode(torch.from_numpy(z[i:i + chunk]).cuda()).cpu().numpy())
    return np.concatenate(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description="betaVAE latent arithmetic between two cohorts of RNA-Seq data (MI355X path)")
    ap.add_argument("--config", type=str, help="JSON config file")
    ap.add_argument("--checkpoint", type=str, required=True, help="File with the trained model's state_dict")
    ap.add_argument("--seed", type=int, default=99, help="Seed of the training run's split")
    ap.add_argument("--type", type=str, default="tissue", help="tissue: the first two CSVs; group: --group_column of the first")
    ap.add_argument("--group_column", type=str, default=None)
    ap.add_argument("--group_a", type=str, default=None)
    ap.add_argument("--group_b", type=str, default=None)
    ap.add_argument("--scaler", type=str, default=None, help="scaler.npz of the training run")
    ap.add_argument("--chunk", type=int, default=256, help="rows per encode / decode call")
    ap.add_argument("--out", type=str, default=None, help="output pickle")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    frames = RT.read_tables(config)
    parts, indices = RT.split_tables(frames, args.seed)
    if args.group_column is not None:
        df = frames[0].iloc[indices[0]["train"]]
        if args.group_column not in df.columns:
            raise SystemExit("the first table has no column %r" % args.group_column)
        if args.group_a is None or args.group_b is None:
            raise SystemExit("--group_column needs --group_a and --group_b")
        col = df[args.group_column].astype(str)
        groups = [df[col == str(args.group_a)], df[col == str(args.group_b)]]
    elif args.type == "tissue":
        if len(frames) < 2:
            raise SystemExit("--type tissue needs two CSVs in path_csv")
        groups = [frames[i].iloc[indices[i]["train"]] for i in (0, 1)]
    else:
        raise SystemExit("choose --type tissue, or --group_column COL --group_a A --group_b B")
    for name, g in zip("ab", groups):
        if g.shape[0] == 0:
            raise SystemExit("group %s has no train rows" % name)
    scaler = RT.scaler_for(config, args.seed, args.scaler, frames=frames)
    features = RT.check_features(config, scaler.mean.shape[0])
    os.makedirs(config["save_dir"], exist_ok=True)
    samples = [np.ascontiguousarray(scaler.transform_frame(g).astype(np.float32)) for g in groups]
    model = RT.model_from_config(config, features)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model = model.set_precision(args.precision).cuda().eval()
    (mu1, lv1, enc1), (mu2, lv2, enc2) = (encode_chunks(model, s, args.chunk) for s in samples)
    c1, c2 = mu1.astype(np.float64).mean(axis=0), mu2.astype(np.float64).mean(axis=0)
    difference1, difference2 = (c1 - c2).astype(np.float32), (c2 - c1).astype(np.float32)
    results = {"z_mu1": mu1, "z_mu2": mu2, "z_logvar1": lv1, "z_logvar2": lv2, "sample1_encod": enc1, "sample2_encod": enc2,
               "sample1": samples[0], "sample2": samples[1],
               "recons_1": decode_chunks(model, enc1 + difference1, args.chunk),
               "recons_2": decode_chunks(model, enc2 + difference2, args.chunk),
               "z_a_to_b": difference1, "z_b_to_a": difference2}
    out = args.out or os.path.join(config["save_dir"], "interpolation_lung_sex_results.pkl")
    with open(out, "wb") as f:
        pickle.dump(results, f)
    print("wrote", out, {k: v.shape for k, v in results.items()})


if __name__ == "__main__":
    main()
