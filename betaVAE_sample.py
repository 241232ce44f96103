#!/usr/bin/env python3
"""Working counterpart of the reference's src/betaVAE_sample.py on the MI355X path: decode N(0, I) latents of a trained betaVAE
-- optionally shifted by the ``z_b_to_a`` direction of a betaVAE_interpolation.py result -- back to expression values.

Flags: --config --checkpoint --seed --num_samples --interpolation PKL [--alpha] [--scaler scaler.npz] [--out].  The model is the
config's (``rna_features``, optional ``encoder_dims`` / ``decoder_dims``); ``model.sample`` runs the eval-mode decoder on the HIP
kernels and ``RnaScaler.inverse_transform`` reverses the standardisation (not the ln, as in the reference).  The scaler is
``--scaler``, else ``scaler.npz`` in the config's ``save_dir`` (betaVAE_training.py writes it), else it is refitted by repeating
the split of the config's ``path_csv`` under the seed -- which is all the reference does.  As there, the generators are seeded
first and the model is built next, so the latents follow the draws of the module's initialisation.  Output: the pickle
``{"generated": ndarray}`` under the reference's file name in ``save_dir`` unless --out is given.
"""
import argparse
import json
import os
import pickle

import numpy as np
import torch

from rna_gan_amd import rna_tables as RT


def main(argv=None):
    ap = argparse.ArgumentParser(description="betaVAE generation of RNA-Seq data (MI355X path)")
    ap.add_argument("--config", type=str, help="JSON config file")
    ap.add_argument("--checkpoint", type=str, required=True, help="File with the trained model's state_dict")
    ap.add_argument("--seed", type=int, default=99, help="Seed for random generation")
    ap.add_argument("--num_samples", type=int, default=64, help="Number of samples to generate.")
    ap.add_argument("--interpolation", type=str, default=None, help="Interpolation file to move between samples")
    ap.add_argument("--alpha", type=float, default=1.0, help="how far along the interpolation direction to move")
    ap.add_argument("--scaler", type=str, default=None, help="scaler.npz of the training run")
    ap.add_argument("--out", type=str, default=None, help="output pickle")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = json.load(f)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    scaler = RT.scaler_for(config, args.seed, args.scaler)
    features = RT.check_features(config, scaler.mean.shape[0])
    os.makedirs(config["save_dir"], exist_ok=True)
    model = RT.model_from_config(config, features)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model = model.set_precision(args.precision).cuda().eval()
    difference = None
    if args.interpolation:
        with open(args.interpolation, "rb") as f:
            difference = np.asarray(pickle.load(f)["z_b_to_a"], dtype=np.float32)
    with torch.no_grad():
        generated = model.sample(args.num_samples, "cuda:0", interpolation=difference, alpha=args.alpha)
    results = {"generated": scaler.inverse_transform(generated.detach().cpu().numpy())}
    out = args.out or os.path.join(config["save_dir"], "generated_samples_interpolation_lung.pkl")
    with open(out, "wb") as f:
        pickle.dump(results, f)
    print("wrote", out, results["generated"].shape)


if __name__ == "__main__":
    main()
