#!/usr/bin/env python3
"""Working counterpart of the reference's src/compute_representation.py on the MI355X path: per patient, the mean feature
vector of its real tiles, of tiles generated from its expression row by the RNA-conditioned GAN, and of tiles of an unconditioned
GAN, written as ``<path_to_save>_real.npy``, ``_vaegan.npy`` and ``_gan.npy``: (P, F) float32 arrays, the reference's dtype.

The reference's flags (--config --gan --vaegan --seed --multiprocessing --sample_size --vae_checkpoint --path_to_save) and its
JSON keys (path_csv, patch_data_path, img_size, rna_features).  What differs, and why:

* Features.  The reference takes Inception-v3 pool features; those weights cannot be obtained offline, so ``--extractor`` is the
  path of a torchvision ``inception_v3`` state dict, or -- the default -- ``discriminator``: the labelled PROXY of
  ``--fd_extractor`` (the trunk of the RNA-conditioned run's critic at native resolution; comparable within one run only).
* Everything between the tiles and the centroids stays on the device: synthesis, resize, extraction and the per-patient means
  (rna_gan_amd.representation: rg_group_sums_update); (P, F) doubles per source come back.
* Generation is the bulk rule of generate_tissue_images.py (``representation.conditioned_noise``: the encoder once, a private
  generator seeded with --seed, groups that mix patients), not the reference's one-patient-at-a-time ``generate_images``, whose
  column standardisation over a single patient removes the conditioning.
* The script also prints what the arrays are for: ``representation.retrieval_scores`` of ``_vaegan`` against ``_real``.
* ``_gan.npy`` is written only with ``--gan``.  ``--multiprocessing`` is accepted and ignored.

Real tiles are ``--sample_size`` random keys per slide drawn under ``--seed`` (rna_gan_amd.data.PatchRNADataset: the reference's
``random.sample`` per slide), read through rna_gan_amd.data / lmdb_ro; unreadable records are skipped, as the reference skips
them.  A patient is a distinct prepared RNA row (``resident.DeviceTileSet.from_dataset``'s rule).  ``--synthetic``: no files
are read -- seeded tiles, rows and network weights of the shapes in the config (``synthetic_patients`` patients, default 8).
"""
import argparse
import json
import os

import numpy as np
import torch

import rna_gan_amd as P


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Compute representation of GAN images (MI355X path)")
    ap.add_argument("--config", type=str, help="JSON config file")
    ap.add_argument("--gan", type=str, default=None, help="checkpoint of the unconditioned GAN (omit: no _gan.npy)")
    ap.add_argument("--vaegan", type=str, default=None, help="checkpoint of the RNA-conditioned GAN")
    ap.add_argument("--seed", type=int, default=99)
    ap.add_argument("--multiprocessing", default=False, action="store_true", help="accepted for compatibility, ignored")
    ap.add_argument("--sample_size", dest="sample_size", type=int, help="tiles per patient, real and generated")
    ap.add_argument("--vae_checkpoint", type=str, default=None, help="checkpoint of the betaVAE")
    ap.add_argument("--path_to_save", type=str, default=None, help="prefix of the three .npy files")
    ap.add_argument("--extractor", type=str, default="discriminator",
                    help="'discriminator' (the labelled proxy) or the path of a torchvision inception_v3 state dict")
    ap.add_argument("--synthetic", action="store_true", help="seeded tiles, RNA rows and weights instead of files")
    args = ap.parse_args(argv)
    if args.config is None or args.path_to_save is None:
        ap.error("--config and --path_to_save are required")
    if args.sample_size is None or args.sample_size < 1:
        ap.error("--sample_size must be at least 1")
    if args.extractor != "discriminator" and not os.path.isfile(args.extractor):
        ap.error("--extractor must be 'discriminator' or the path of an inception_v3 state dict (no such file: %s)" % args.extractor)
    if not args.synthetic and (args.vaegan is None or args.vae_checkpoint is None):
        ap.error("--vaegan and --vae_checkpoint are required without --synthetic")
    return args


def _file_inputs(args, config, device):
    from rna_gan_amd.gan_utils import load_torchgan_trainer, resident_training_set
    ts = resident_training_set(config, args.seed, args.sample_size, device)
    print("Real tiles on {}: {} tiles of {} patients, {} unreadable records skipped".format(device, len(ts), ts.rna.shape[0], ts.dropped))
    features = int(config.get("rna_features", ts.rna.shape[1]))
    bv = P.betaVAE(features, 2048, [6000, 4000, 2048], [4000, 6000], beta=0.0005)
    bv.load_state_dict(torch.load(args.vae_checkpoint, map_location="cpu"))
    vaegan = load_torchgan_trainer(args.vaegan, device=str(device))
    gan = load_torchgan_trainer(args.gan, device=str(device)).generator if args.gan is not None else None
    return ts, vaegan.generator, vaegan.discriminator, bv.to(device), gan


def run(args):
    """The three (two without --gan) sets of centroids as (P, F) fp64 device tensors under "real", "conditioned" and
    "unconditioned"; writes the .npy files and prints the retrieval scores."""
    from rna_gan_amd import representation as RP
    from rna_gan_amd import synth
    from rna_gan_amd.metrics import feature_extractor
    with open(args.config) as f:
        config = json.load(f)
    print(10 * "-"); print("Config for this experiment \n"); print(config); print(10 * "-")
    device = torch.device("cuda:0")
    if args.synthetic:
        ts, G, D, bv, gan = synth.evaluation_inputs(config, args.sample_size, args.seed, device, second_generator=args.gan is not None)
    else:
        ts, G, D, bv, gan = _file_inputs(args, config, device)
    extract, resize = feature_extractor(args.extractor, D, device)
    reps = RP.patient_representations(extract, real=ts, conditioned=G, unconditioned=gan, betavae=bv, gene_exp=ts.rna,
                                      tiles_per_patient=args.sample_size, seed=args.seed, resize=resize)
    for key, name in (("real", "real"), ("conditioned", "vaegan"), ("unconditioned", "gan")):
        if key in reps:
            np.save(args.path_to_save + "_%s.npy" % name, reps[key].float().cpu().numpy())
    patients = reps["real"].shape[0]
    if patients >= 2:
        rank, _ = RP.match_ranks(reps["conditioned"], reps["real"])
        print("Conditioning retrieval, {} patients x {} tiles ({} features): {}".format(
            patients, args.sample_size, "discriminator proxy" if resize is None else "inception", RP.retrieval_scores(rank, patients)))
    return reps


if __name__ == "__main__":
    run(parse_args())
