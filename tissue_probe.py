#!/usr/bin/env python3
"""Counterpart, on FROZEN features, of the reference's src/ml_experiments.py on the MI355X path: is a tissue classifier helped by
tiles generated from gene expression?

What the reference asks: it fine-tunes a ResNet-50 (optionally from SimCLR weights) to classify the tissue of a tile under
``StratifiedKFold(5, shuffle=True)``, on real tiles, on generated tiles and on both, and reports accuracy and
``f1_score(average="weighted")``.  That script does not parse.  What is mirrored here: the three training
settings, the 5-fold stratified cross-validation over the real tiles, accuracy, weighted F1 and the confusion matrices.  What is
NOT mirrored, plainly: no ResNet fine-tuning and no SimCLR weights -- the classifier is a linear probe (multinomial logistic
regression, rna_gan_amd.linprobe, fitted on the device in fp64) on the features of ``--extractor``: the critic's trunk at native
resolution (the default, the labelled proxy of --fd_extractor) or a torchvision inception_v3 state dict.  The numbers answer the
reference's question for a frozen representation, not for a fine-tuned network.

  real                 the probe cross-validated on the real tiles (every tile tested once, by a probe that did not see it)
  synthetic            TSTR: the probe trained on generated tiles alone -- ``--sample_size`` tiles per expression row, each
                       labelled with its row's tissue -- tested on all real tiles
  real_plus_synthetic  the same folds as ``real``, every training fold enlarged by all generated tiles

``<out_dir>/probe.json`` holds, per setting, "accuracy", "weighted_f1" and "confusion" ([true][predicted]), next to the tissue
codes and the sizes.  The tissue of a tile is the index of its slide table in the config's ``path_csv`` (rna_gan_amd.data); the
generated tiles come from ``representation.conditioned_noise`` under ``--seed``.  The betaVAE has the reference's sizes unless the
config carries ``encoder_dims`` / ``decoder_dims`` (the keys of betaVAE_training.py).  ``--synthetic``: no files are read -- seeded
tiles, rows (two tissues, alternating) and network weights of the shapes in the config (``synthetic_patients``, default 8).
"""
import argparse
import json
import os

import numpy as np
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Tissue probe on real, generated and mixed training tiles (MI355X path)")
    ap.add_argument("--config", type=str, help="JSON config file")
    ap.add_argument("--checkpoint", type=str, default=None, help="checkpoint of the RNA-conditioned GAN")
    ap.add_argument("--vae_checkpoint", type=str, default=None, help="checkpoint of the betaVAE")
    ap.add_argument("--out_dir", type=str, default=None, help="directory that receives probe.json")
    ap.add_argument("--seed", type=int, default=99)
    ap.add_argument("--sample_size", type=int, default=8, help="tiles per expression row, real and generated")
    ap.add_argument("--folds", type=int, default=5, help="folds of the stratified cross-validation")
    ap.add_argument("--l2", type=float, default=1e-3, help="the probe's penalty")
    ap.add_argument("--extractor", type=str, default="discriminator",
                    help="'discriminator' (the labelled proxy) or the path of a torchvision inception_v3 state dict")
    ap.add_argument("--synthetic", action="store_true", help="seeded tiles, RNA rows and weights instead of files")
    args = ap.parse_args(argv)
    if args.config is None or args.out_dir is None:
        ap.error("--config and --out_dir are required")
    if args.sample_size < 1:
        ap.error("--sample_size must be at least 1")
    if args.folds < 2:
        ap.error("--folds must be at least 2")
    if not (np.isfinite(args.l2) and args.l2 > 0):
        ap.error("--l2 must be finite and > 0")
    if args.extractor != "discriminator" and not os.path.isfile(args.extractor):
        ap.error("--extractor must be 'discriminator' or the path of an inception_v3 state dict (no such file: %s)" % args.extractor)
    if not args.synthetic and (args.checkpoint is None or args.vae_checkpoint is None):
        ap.error("--checkpoint and --vae_checkpoint are required without --synthetic")
    return args


def _file_inputs(args, config, device):
    from rna_gan_amd.gan_utils import load_torchgan_trainer, resident_training_set
    from rna_gan_amd.rna_tables import model_from_config
    ts = resident_training_set(config, args.seed, args.sample_size, device)
    print("Real tiles on {}: {} tiles of {} expression rows, {} unreadable records skipped".format(device, len(ts), ts.rna.shape[0],
                                                                                                 ts.dropped))
    features = int(config.get("rna_features", ts.rna.shape[1]))
    # the reference's sizes (2048, [6000, 4000, 2048], [4000, 6000]) unless the config's optional encoder_dims / decoder_dims say
    # otherwise -- the keys betaVAE_training.py builds its model from, so a checkpoint trained with other sizes loads
    bv = model_from_config(config, features)
    bv.load_state_dict(torch.load(args.vae_checkpoint, map_location="cpu"))
    gan = load_torchgan_trainer(args.checkpoint, device=str(device))
    if int(gan.generator.encoding_dims) != int(bv.z_dim):
        raise SystemExit("tissue_probe: the generator takes %d-d noise, the betaVAE of this config encodes to %d"
                         % (int(gan.generator.encoding_dims), int(bv.z_dim)))
    return ts, gan.generator, gan.discriminator, bv.to(device)


def _report(pred, y, C):
    from rna_gan_amd import linprobe as LP
    return {"accuracy": LP.accuracy(pred, y), "weighted_f1": LP.weighted_f1(pred, y, C), "confusion": LP.confusion_matrix(pred, y, C).tolist()}


def run(args):
    """the three settings as a dictionary; writes <out_dir>/probe.json"""
    from rna_gan_amd import linprobe as LP
    from rna_gan_amd import synth
    from rna_gan_amd.metrics import _eval_mode, feature_extractor
    from rna_gan_amd.representation import tile_features
    with open(args.config) as f:
        config = json.load(f)
    print(10 * "-"); print("Config for this experiment \n"); print(config); print(10 * "-")
    device = torch.device("cuda:0")
    if args.synthetic:
        ts, G, D, bv, _ = synth.evaluation_inputs(config, args.sample_size, args.seed, device, tissues=True)
    else:
        ts, G, D, bv = _file_inputs(args, config, device)
    extract, resize = feature_extractor(args.extractor, D, device)
    try:      # one tissue per expression row, at least two tissues, enough tiles of each for the folds
        classes, y_real, row_label = LP.row_tissues(ts.labels.round().long(), ts.row_of, ts.rna.shape[0], args.folds)
    except ValueError as e:
        raise SystemExit("tissue_probe: %s" % e)
    C = len(classes)
    with torch.no_grad(), _eval_mode(G, D):
        feats = tile_features(extract, real=(ts.tiles, ts.row_of), conditioned=G, betavae=bv, gene_exp=ts.rna,
                              tiles_per_patient=args.sample_size, seed=args.seed, resize=resize)
    real = feats["real"][0]
    fake, fake_rows = feats["conditioned"]
    y_fake = row_label[fake_rows.cpu().numpy().astype(np.int64)]
    out = {"tissues": [int(c) for c in classes], "real_tiles": int(real.shape[0]), "generated_tiles": int(fake.shape[0]),
           "features": int(real.shape[1]), "extractor": "discriminator proxy" if resize is None else "inception", "folds": args.folds,
           "l2": args.l2, "seed": args.seed}
    pred, _, _ = LP.cross_validated(real, y_real, C, args.folds, args.seed, args.l2)
    out["real"] = _report(pred, y_real, C)
    out["synthetic"] = _report(LP.predict(LP.fit(fake, y_fake, C, l2=args.l2), real), y_real, C)
    pred, _, _ = LP.cross_validated(real, y_real, C, args.folds, args.seed, args.l2, extra=(fake, y_fake))
    out["real_plus_synthetic"] = _report(pred, y_real, C)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "probe.json"), "w") as f:
        json.dump(out, f, indent=1)
    for key in ("real", "synthetic", "real_plus_synthetic"):
        print("{:<20s} accuracy {:.4f}  weighted F1 {:.4f}".format(key, out[key]["accuracy"], out[key]["weighted_f1"]))
    return out


if __name__ == "__main__":
    run(parse_args())
