#!/usr/bin/env python3
"""Is a trained generator reproducing its training tiles?  (rna_gan_amd.nearest on the MI355X path)

    audit_memorisation.py --checkpoint G.model --config CONFIG [--vae_checkpoint VAE] --samples 2048 --factor 4 --k 4 --out_dir DIR

--config is the training run's JSON (path_csv, patch_data_path, img_size): the training tiles are read once, as the trainer's
--resident 1 reads them (--num_patches tiles per slide), and kept on the device as uint8.  --samples tiles are generated -- with
--vae_checkpoint from the expression rows of the training slides, the same number per slide (rna_gan_amd.gan_utils.generate_tiles);
without it from standard normal noise -- and every one is searched against all training tiles by int8 block-mean descriptors
(--factor) on the device: exact integer distances, ties to the lower training index.  --d4 1 (the default) searches each sample
under all eight symmetries of the square, which a generator trained with --augment d4 may have applied to a memorised tile.

DIR/nearest.csv   one row per generated tile: generated index, the k training indices and squared distances, loo_d2 (from the
                  nearest training tile to ITS nearest other training tile), copied (d2_0 < loo_d2), exact (d2_0 == 0)
DIR/nearest.png   the 16 generated tiles with the smallest d2_0, each beside its k nearest training tiles
and a summary line: copy_rate, exact, min_d2, median_d2.  A generator that does not memorise has a copy_rate near 0.5 (a sample
of the training distribution is as often closer to a training tile as that tile's own neighbour is, as not); copying pushes it
towards 1.  An exact duplicate pair inside the training set has loo_d2 = 0: a copy of either is never ``copied`` and shows in
``exact``.

--synthetic runs without files: seeded random weights and uniform random training tiles, like every other CLI here.
"""
import argparse
import json
import os

import numpy as np
import torch

FLAGS = [
    ("--config", str, None, "the training run's JSON config (path_csv, patch_data_path, img_size)"),
    ("--checkpoint", str, None, "generator checkpoint (a Trainer .model file)"),
    ("--vae_checkpoint", str, None, "betaVAE state dict: the generator is conditioned on the training slides' expression rows"),
    ("--rna_features", int, 19198, "number of genes (--vae_checkpoint; read from --config when present)"),
    ("--num_patches", int, 250, "tiles per slide of the training set, as the training run's"),
    ("--samples", int, 2048, "generated tiles to audit"),
    ("--factor", int, 4, "the descriptor averages a tile over blocks of this size (1, 2, 4, 8, 16 or 32)"),
    ("--k", int, 4, "nearest training tiles reported per generated tile (1..8)"),
    ("--d4", int, 1, "1 = search every sample under all eight symmetries of the square, 0 = as generated"),
    ("--out_dir", str, None, "output directory"),
    ("--g_ema", int, 0, "1 = the checkpoint's averaged generator (generator_ema)"),
    ("--precision", str, "bf16", "bf16, fp16 or fp32"),
    ("--seed", int, 0, "seed of the noise"),
    ("--img_size", int, 256, "--synthetic: tile edge"),
    ("--synthetic_tiles", int, 512, "--synthetic: training tiles"),
]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Audit a generator for memorised training tiles (MI355X path)")
    for flag, typ, default, text in FLAGS:
        ap.add_argument(flag, type=typ, default=default, help=text)
    ap.add_argument("--synthetic", action="store_true", help="seeded random weights and random training tiles instead of the files")
    args = ap.parse_args(argv)
    if not args.out_dir:
        ap.error("--out_dir is required")
    if not args.synthetic:
        for flag in ("checkpoint", "config"):
            if getattr(args, flag) is None:
                ap.error("--%s is required without --synthetic" % flag)
    if args.samples < 1:
        ap.error("--samples must be >= 1")
    from rna_gan_amd.gan_utils import check_flags
    from rna_gan_amd.nearest import FACTORS
    if args.factor not in FACTORS:
        ap.error("--factor must be 1, 2, 4, 8, 16 or 32")
    if not 1 <= args.k <= 8:
        ap.error("--k must be in 1..8")
    check_flags(ap, args, binary=("d4", "g_ema"))
    if args.num_patches < 1 or args.img_size < 1 or args.synthetic_tiles < 2:
        ap.error("--num_patches and --img_size must be positive, --synthetic_tiles at least 2")
    return args


def training_set(args, config, device, with_rna):
    """The training tiles as a resident.DeviceTileSet (with the slides' expression rows when the generator is conditioned)."""
    if args.synthetic:
        from rna_gan_amd.resident import DeviceTileSet
        from rna_gan_amd.synth import synthetic_tiles_u8
        return DeviceTileSet.from_tensors(synthetic_tiles_u8(args.synthetic_tiles, args.img_size, args.seed + 1), device=device)
    from rna_gan_amd.gan_utils import resident_training_set
    return resident_training_set(config, args.seed, args.num_patches, device, with_rna=with_rna, workers=4)


def generated_tiles(args, trainer, betavae, ts, device):
    """uint8 [samples][3][S][S] on the device."""
    from rna_gan_amd.export import tiles_u8
    from rna_gan_amd.gan_utils import generate_tiles, synthesize
    if betavae is not None:
        P_ = int(ts.rna.shape[0])
        per = (args.samples + P_ - 1) // P_
        out = None
        for p, t, a in generate_tiles(trainer, ts.rna.cpu(), per, betavae, seed=args.seed, ema=bool(args.g_ema), layout="nchw"):
            if out is None:
                out = np.empty((P_ * per,) + a.shape[1:], dtype=np.uint8)
            out[t * P_ + p] = a                             # tile-major: the first `samples` rows cover the slides evenly
        return torch.from_numpy(out[:args.samples]).to(device)
    G = trainer.generator_ema if args.g_ema else trainer.generator
    z = torch.randn(args.samples, int(G.encoding_dims), generator=torch.Generator().manual_seed(args.seed)).to(device)
    return torch.cat([tiles_u8(synthesize(G, c, chunk=256), layout="nchw") for c in torch.split(z, 256)])


def compose_sheet(generated, neighbours):
    """generated (R, 3, S, S) and neighbours (R, k, 3, S, S) uint8 -> one (R * S, (k + 1) * S + gap, 3) image: per row the
    generated tile, a white gap, its k nearest training tiles."""
    R_, k = neighbours.shape[:2]
    S, gap = generated.shape[-1], max(generated.shape[-1] // 16, 1)
    sheet = np.full((R_ * S, (k + 1) * S + gap, 3), 255, dtype=np.uint8)
    for r in range(R_):
        sheet[r * S:(r + 1) * S, :S] = generated[r].transpose(1, 2, 0)
        for j in range(k):
            x0 = S + gap + j * S
            sheet[r * S:(r + 1) * S, x0:x0 + S] = neighbours[r, j].transpose(1, 2, 0)
    return sheet


def run(args, trainer=None, betavae=None, tile_set=None):
    """The work of the CLI.  trainer / betavae / tile_set: handed in (tests); otherwise built from the arguments.  Returns
    (the AuditResult, the list of paths written)."""
    from PIL import Image
    from rna_gan_amd.nearest import TrainIndex, audit
    device = torch.device("cuda", 0)
    config = {}
    if args.config:
        with open(args.config) as f:
            config = json.load(f)
        args.rna_features = int(config.get("rna_features", args.rna_features))
    if trainer is None:
        from rna_gan_amd.gan_utils import build_models
        trainer, betavae = build_models(args, device)
    ts = tile_set if tile_set is not None else training_set(args, config, device, betavae is not None)
    if betavae is not None and ts.rna is None:
        raise SystemExit("--vae_checkpoint needs a training set with expression rows")
    index = TrainIndex(ts, factor=args.factor)
    gen = generated_tiles(args, trainer, betavae, ts, device)
    if tuple(gen.shape[1:]) != tuple(ts.tiles.shape[1:]):
        raise SystemExit("the generator makes %s tiles, the training set holds %s" % (tuple(gen.shape[1:]), tuple(ts.tiles.shape[1:])))
    res = audit(gen, index, k=args.k, d4=bool(args.d4))
    os.makedirs(args.out_dir, exist_ok=True)
    csv = os.path.join(args.out_dir, "nearest.csv")
    with open(csv, "w") as f:
        f.write(",".join(["generated"] + ["index_%d" % j for j in range(args.k)] + ["d2_%d" % j for j in range(args.k)] +
                         ["loo_d2", "copied", "exact"]) + "\n")
        for g in range(res.d2.shape[0]):
            f.write(",".join([str(g)] + [str(int(v)) for v in res.index[g]] + [str(int(v)) for v in res.d2[g]] +
                             [str(int(res.loo_d2[g])), str(int(res.copied[g])), str(int(res.exact[g]))]) + "\n")
    closest = np.argsort((res.d2[:, 0] << 32) | np.arange(res.d2.shape[0]), kind="stable")[:16]
    rows = torch.from_numpy(res.index[closest].reshape(-1)).to(ts.device)
    neighbours = ts.tiles.index_select(0, rows).cpu().numpy().reshape((len(closest), args.k) + tuple(ts.tiles.shape[1:]))
    png = os.path.join(args.out_dir, "nearest.png")
    Image.fromarray(compose_sheet(gen[torch.from_numpy(closest).to(gen.device)].cpu().numpy(), neighbours)).save(png)
    print("memorisation audit: %d generated against %d training tiles, factor %d, k %d, d4 %d: %s"
          % (gen.shape[0], len(index), args.factor, args.k, args.d4, json.dumps(res.summary())))
    return res, [csv, png]


def main(argv=None):
    for path in run(parse_args(argv))[1]:
        print(path)


if __name__ == "__main__":
    main()
