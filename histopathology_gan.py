#!/usr/bin/env python3
"""Working counterpart of the reference CLI (src/histopathology_gan.py) on the MI355X path.

Same flags (--config --checkpoint --seed --image_dir --model_dir --num_epochs --num_patches
--gan_type --loss_type) and the same JSON keys (path_csv, patch_data_path, save_dir, img_size,
[flag, encoder_checkpoint, bag_size]); the model/optimizer dictionary, loss selection, Trainer call
and checkpoint naming follow src/histopathology_gan.py:175-192,248-278,298-314.

The reference script itself cannot start (absent modules wsi_model/biggan/sagan).  Real data goes
through rna_gan_amd.data (the reference's tile-record format, per-slide sampling and RNA log / StandardScaler
preparation; slide databases as LMDB files when the ``lmdb`` package is installed, or as directory stores);
``--synthetic`` trains on synthetic tiles / RNA rows of the right shapes (what bench.py measures).  Extra flags: --batch_size (reference hard-codes 8),
--precision, --betavae_checkpoint, --steps_per_epoch; --device_transform 1 hands the uint8 tiles to the device and normalises
them there, --augment d4 applies one of the eight symmetries of the square per real sample (rna_gan_amd.augment);
--resident 1 keeps the rank's training tiles on the device as uint8 and forms every batch there (rna_gan_amd.resident); with it, --mem_samples N audits N generated tiles per epoch for memorised
training tiles (rna_gan_amd.metrics.Memorisation; data parallel: against the rank's own shard).
"""
import argparse
import datetime
import json
import os

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL on this driver stack (before torch initialises HIP)

import numpy as np
import torch
import torch.nn as nn
from torch.optim import Adam
from torch.utils.data import DataLoader, Dataset

import rna_gan_amd as P
from rna_gan_amd import dist as D_


class SyntheticTiles(Dataset):
    """uint8 uniform tiles -> float -> (x-0.5)/0.5 (src/histopathology_gan.py:106-109) and N(0,1) RNA rows
    (StandardScaler output, :148-151) with 16 distinct rows (tiles of a slide share RNA).  ``as_u8``: the same draws as the
    uint8 tiles themselves (--device_transform 1: normalised on the device)."""

    def __init__(self, n, img_size, rna_features, with_rna, seed, as_u8=False):
        self.n, self.s, self.f, self.with_rna, self.as_u8 = n, img_size, rna_features, with_rna, as_u8
        rng = np.random.default_rng(seed)
        self.rows = torch.from_numpy(rng.normal(size=(16, rna_features)).astype(np.float32))
        self.seed = seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.default_rng([self.seed, i])
        img = torch.from_numpy(rng.integers(0, 256, size=(3, self.s, self.s), dtype=np.uint8))
        if not self.as_u8:
            img = (img.float() / 255.0 - 0.5) / 0.5
        if self.with_rna:
            return {"image": img, "rna_data": self.rows[i % 16], "labels": torch.tensor(0.0)}
        return img, torch.tensor(0.0)


# (flag, type, default, help) -- the reference's flag set (src/histopathology_gan.py:54-72) + this build's extras
REFERENCE_FLAGS = [
    ("--config", str, None, "JSON config file"),
    ("--checkpoint", str, None, "File with the checkpoint to start with"),
    ("--seed", int, 99, "Seed for random generation"),
    ("--image_dir", str, "images", "Image dir to save image"),
    ("--model_dir", str, "./model/gan", "Image dir to save model checkpoints"),
    ("--num_epochs", int, None, "Number of epochs to train the model"),
    ("--num_patches", int, 250, "Number of tiles to use per slide"),
    ("--gan_type", str, "dcgan", "Architecture to use"),
    ("--loss_type", str, "wgangp", "Loss type to use"),
]
EXTRA_FLAGS = [
    ("--sync_stats", int, 0, "data parallel: 1 = BatchNorm / latent / penalty statistics over the GLOBAL batch (exact "
                              "single-process semantics, no HIP graphs), 0 = rank-local statistics (plain DDP)"),
    ("--batch_size", int, 8, "per-process batch (the reference hard-codes 8, :94)"),
    ("--precision", str, "bf16", "bf16 (MFMA kernels), fp16 (the same kernels built for IEEE fp16 storage, loss-scaled backward) or fp32 (parity mode)"),
    ("--betavae_checkpoint", str, "checkpoints/betavae_training_tissues/model_dict_best.pt", "frozen betaVAE weights"),
    ("--steps_per_epoch", int, 100, "synthetic dataset length / batch"),
    ("--loss_scaling", str, "static", "fp16 only: static (fixed scale RNAGAN_F16_LOSS_SCALE) or dynamic (GradScaler-style: a step "
                                      "with a non-finite gradient is skipped and the scale halved; it grows after clean steps)"),
    ("--critic_batchnorm", int, 1, "0 = BatchNorm-free critic (DCGANDiscriminator(batchnorm=False): biased convs, what a WGAN-GP "
                                   "recipe uses -- the penalty is per input and train-mode BatchNorm couples the batch)"),
    ("--g_ema", float, 0.0, "decay in [0, 1) of an exponential moving average of the generator's weights, kept on the device "
                            "inside the optimizer step and saved / sampled next to the generator (0 = off)"),
    ("--g_ema_warmup", int, 1, "1 = the average's decay is min(g_ema, (1 + t) / (10 + t)) at generator step t, 0 = constant"),
    ("--fd_samples", int, 0, "evaluate a Frechet distance after every epoch (rna_gan_amd.metrics.FrechetDistance, logged in the "
                             "checkpoint's metric_logs): the first N items of the dataset are held on the device as the real set "
                             "and N images are generated from fixed noise (0 = off)"),
    ("--fd_extractor", str, "discriminator", "features of --fd_samples: 'discriminator' (the labelled proxy: the critic's trunk, "
                                             "comparable within one run only) or the path of a torchvision inception_v3 state dict"),
    ("--kid_samples", int, 0, "evaluate a kernel distance (KID: the unbiased MMD^2 under the cubic polynomial kernel, "
                              "rna_gan_amd.metrics.KernelDistance) after every epoch on the first N items of the dataset and N "
                              "generated images, features of --fd_extractor; with --fd_samples N the two metrics share the real "
                              "set and the noise (0 = off)"),
    ("--kid_subsets", int, 0, "--kid_samples: log the mean over K random row subsets instead of the full-set estimate (the "
                              "published convention is 100; 0 = the full-set estimate)"),
    ("--kid_subset_size", int, 1000, "--kid_subsets: rows per subset (clamped to the number of samples)"),
    ("--pr_samples", int, 0, "evaluate precision, recall, density and coverage (k-nearest-neighbour manifold estimates, "
                             "rna_gan_amd.metrics.PrecisionRecall) after every epoch on the first N items of the dataset and N "
                             "generated images, features of --fd_extractor; with --fd_samples N and / or --kid_samples N the "
                             "metrics share the real set and the noise (0 = off, otherwise at least --pr_k + 1)"),
    ("--pr_k", int, 5, "--pr_samples: the neighbourhood size k (1..16)"),
    ("--pr_report", str, "recall", "--pr_samples: which of precision, recall, density, coverage is logged in metric_logs (all "
                                   "four are kept per epoch in the checkpointed metric's history)"),
    ("--qc_samples", int, 0, "evaluate the tissue yield (rna_gan_amd.metrics.TissueYield) after every epoch: the fraction of N "
                             "generated tiles that the reference tiler's acceptance rule keeps -- a tissue mask over more than "
                             "20 % of the tile, not low-contrast (rna_gan_amd.tissue, on the device; no real tiles are judged); "
                             "with another metric over N samples it shares the noise (0 = off)"),
    ("--div_samples", int, 0, "evaluate the pixel-space diversity (rna_gan_amd.metrics.PairDiversity) after every epoch: the mean "
                              "MS-SSIM over random pairs of N generated tiles, next to the same pairs of the first N items of the "
                              "dataset (turned back to bytes); generated pairs clearly more similar than real ones, or a sudden "
                              "rise between epochs, mean mode collapse; no feature extractor is involved; with another metric "
                              "over N samples it shares the noise (0 = off, otherwise at least 2)"),
    ("--div_pairs", int, 0, "--div_samples: how many random pairs (0 = as many as samples)"),
    ("--cf_patients", int, 0, "--loss_type wganvae only: evaluate the conditioning fidelity "
                              "(rna_gan_amd.metrics.ConditioningFidelity) after every epoch over the first P distinct RNA rows of "
                              "the dataset: per patient, the mean features (--fd_extractor) of its real tiles and of --cf_tiles "
                              "tiles generated from its row, then the rank of its own real centroid among the P for every "
                              "generated one (0 = off, otherwise at least 2)"),
    ("--cf_tiles", int, 8, "--cf_patients: tiles per patient -- generated, and at most that many readable real ones"),
    ("--cf_report", str, "top1", "--cf_patients: which of top1, top5, mrr, median_rank is logged in metric_logs (all are kept per "
                                 "epoch in the checkpointed metric's history)"),
    ("--device_transform", int, 0, "1 = the loader hands over uint8 tiles (a quarter of the host-to-device bytes) and one launch "
                                   "normalises them on the device, bit-identical to the host transform "
                                   "(rna_gan_amd.augment.InputTransform); 0 = the reference's host transform"),
    ("--augment", str, "none", "none, or d4: every real sample of a training batch is mapped by one of the eight symmetries of "
                               "the square (four rotations, each with or without a flip) drawn per sample from --seed, the rank "
                               "and the batch counter, in the same launch; works on the float batch under --device_transform 0"),
    ("--resident", int, 0, "1 = the training set is decoded once and kept on the device as uint8 (rna_gan_amd.resident): every "
                           "batch is gathered, normalised and -- under --augment d4 -- transformed there by one launch, without "
                           "loader workers or a per-batch host-to-device copy; implies the uint8 datasets; unreadable records "
                           "are dropped once, every batch is full; the set must fit the device (--resident_max_gb)"),
    ("--resident_max_gb", float, 0.0, "--resident 1: the memory budget of the set in GiB (0 = the device's free memory minus "
                                      "8 GiB); a set that needs more is refused before anything is uploaded"),
    ("--mem_samples", int, 0, "--resident 1 only: audit memorisation (rna_gan_amd.metrics.Memorisation) after every epoch: the "
                              "exact nearest training tiles of N generated tiles among the rank's resident set, by int8 "
                              "block-mean descriptors on the device (rna_gan_amd.nearest); logs the fraction of samples that are "
                              "closer to a training tile than any other training tile is (0 = off)"),
    ("--mem_factor", int, 4, "--mem_samples: the descriptor averages the tile over blocks of this size (1, 2, 4, 8, 16 or 32)"),
    ("--mem_d4", int, 1, "--mem_samples: 1 = search every sample under all eight symmetries of the square (what --augment d4 "
                         "can teach the generator to return), 0 = as generated"),
]


def make_collate_fn(with_rna: bool, world: int):
    """The reference's collate_fn (src/histopathology_gan.py:24-34): drop records whose tile could not be read.  Data
    parallel (world > 1): every rank must see the SAME batch size -- the gathered G.0 gradient factors and the captured step
    graphs are sized by it, and each train_op issues a collective -- so the dropped records are replaced by repeating this
    batch's readable ones instead of shrinking the batch."""
    def collate_fn(batch):
        img = (lambda b: b["image"]) if with_rna else (lambda b: b[0])
        want = len(batch)
        batch = [b for b in batch if img(b) is not None]
        if world > 1 and len(batch) < want:
            if not batch:
                raise RuntimeError("data parallel: a batch with no readable tile record cannot be equalised across ranks")
            batch = (batch * ((want + len(batch) - 1) // len(batch)))[:want]
        return torch.utils.data.dataloader.default_collate(batch)
    return collate_fn


def shard_indices(n_items: int, rank: int, world: int, batch_size: int):
    """Indices of rank ``rank``'s shard of a list of n_items: strided (rank, rank + world, ...), truncated so that EVERY rank
    gets the same number of items and that number is a multiple of the batch size (equal batch counts on all ranks)."""
    per_rank = (n_items // world) // batch_size * batch_size
    return list(range(rank, n_items, world))[:per_rank]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="GANs training on histology data (MI355X path)")
    for flag, typ, default, text in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(flag, type=typ, default=default, help=text)
    ap.add_argument("--synthetic", action="store_true", help="train on synthetic tiles / RNA rows")
    args = ap.parse_args(argv)
    from rna_gan_amd.gan_utils import check_flags
    from rna_gan_amd.metrics import ConditioningFidelity, PrecisionRecall
    from rna_gan_amd.nearest import FACTORS
    check_flags(ap, args, binary=("g_ema_warmup", "device_transform", "resident", "mem_d4"), precision=False)   # (--precision: main())
    if not 0.0 <= args.g_ema < 1.0:
        ap.error("--g_ema must be in [0, 1)")
    if args.fd_samples < 0 or args.fd_samples == 1:
        ap.error("--fd_samples must be 0 (off) or at least 2 (a covariance needs two samples)")
    if args.fd_extractor != "discriminator" and not os.path.isfile(args.fd_extractor):
        ap.error("--fd_extractor must be 'discriminator' or the path of an inception_v3 state dict (no such file: %s)"
                 % args.fd_extractor)
    if args.kid_samples < 0 or args.kid_samples == 1:
        ap.error("--kid_samples must be 0 (off) or at least 2 (the unbiased estimator divides by n - 1)")
    if args.kid_subsets < 0:
        ap.error("--kid_subsets must be >= 0")
    if args.kid_subset_size < 2:
        ap.error("--kid_subset_size must be at least 2")
    if not 1 <= args.pr_k <= 16:
        ap.error("--pr_k must be in 1..16")
    if args.pr_samples < 0 or 0 < args.pr_samples <= args.pr_k:
        ap.error("--pr_samples must be 0 (off) or at least --pr_k + 1 (a k-th neighbour needs k other samples)")
    if args.qc_samples < 0 or args.qc_samples == 1:
        ap.error("--qc_samples must be 0 (off) or at least 2")
    if args.div_samples < 0 or args.div_samples == 1:
        ap.error("--div_samples must be 0 (off) or at least 2 (a pair needs two tiles)")
    if args.div_pairs < 0:
        ap.error("--div_pairs must be >= 0")
    if args.pr_report not in PrecisionRecall.REPORTS:
        ap.error("--pr_report must be precision, recall, density or coverage")
    if args.cf_patients < 0 or args.cf_patients == 1:
        ap.error("--cf_patients must be 0 (off) or at least 2 (a rank among fewer than two patients says nothing)")
    if args.cf_patients > 0 and args.loss_type != "wganvae":
        ap.error("--cf_patients needs --loss_type wganvae (only that generator is conditioned on RNA)")
    if args.cf_tiles < 1:
        ap.error("--cf_tiles must be at least 1")
    if args.cf_report not in ConditioningFidelity.REPORTS:
        ap.error("--cf_report must be top1, top5, mrr or median_rank")
    if args.augment not in ("none", "d4"):
        ap.error("--augment must be none or d4")
    if args.resident_max_gb < 0:
        ap.error("--resident_max_gb must be >= 0")
    if args.mem_samples < 0:
        ap.error("--mem_samples must be >= 0")
    if args.mem_samples > 0 and not args.resident:
        ap.error("--mem_samples needs --resident 1: the audit searches the training tiles where they are kept on the device")
    if args.mem_factor not in FACTORS:
        ap.error("--mem_factor must be 1, 2, 4, 8, 16 or 32")
    return args


def metric_inputs(args, n_samples, flag, ds, losses, device, holder):
    """(real, extractor, noise, batch_size) of a per-epoch metric over the first ``n_samples`` items of ``ds`` (held on the
    device).  wganvae: the fake noise is built ONCE from those items' RNA rows by generate_images' rule -- a uniform draw (here
    from a private generator, never the global one) plus the encoder's mean, standardised per column by rg_latent_prep over
    the metric's own rows (no collective).  ``holder["trainer"]`` is filled in once the Trainer exists: the noise needs its
    generator.  ``holder`` also keeps what is built here, so two metrics over the same number of samples share one device copy of
    the real set and one noise callable, and all metrics share one extractor."""
    from rna_gan_amd.representation import latent_prep
    extractor = shared_extractor(args, device, holder)
    shared = holder.setdefault("metric_inputs", {})
    if n_samples in shared:
        return shared[n_samples]
    with_rna = args.loss_type == "wganvae"
    items = [ds[i] for i in range(min(n_samples, len(ds)))]
    image_of = (lambda b: b["image"]) if with_rna else (lambda b: b[0])
    items = [b for b in items if image_of(b) is not None]
    if len(items) < 2:
        raise SystemExit("%s: fewer than 2 readable tiles among the first %d items" % (flag, n_samples))
    real = torch.stack([image_of(b) for b in items])
    if real.dtype == torch.uint8:                          # --device_transform 1: unaugmented, scaled as the training batches
        real = holder["input_transform"].normalize(real, device)
    real = real.to(device)
    noise = None
    if with_rna:
        rna = torch.stack([b["rna_data"] for b in items])
        private = torch.Generator().manual_seed(args.seed)
        cache = {}

        def noise(n):
            if "z" not in cache:
                trainer = holder["trainer"]
                betavae = losses[0].betavae.to(device)
                E = trainer.generator.encoding_dims
                u = torch.empty(n, E).uniform_(-0.3, 0.3, generator=private).to(device).contiguous()
                was_training = betavae.training
                betavae.eval()                             # the frozen encoder: no dropout draw, no running-statistics update
                with torch.no_grad():
                    z = betavae.encode(rna.to(device))[0].detach().float().contiguous()
                betavae.train(was_training)
                cache["z"] = latent_prep(u, z)
            return cache["z"]
    shared[n_samples] = (real, extractor, noise, min(256, len(items)))
    return shared[n_samples]


def shared_extractor(args, device, holder):
    """--fd_extractor as the metrics take it, built once and kept in ``holder``: every per-epoch metric uses this one."""
    if "extractor" not in holder:
        from rna_gan_amd.fid import inception_features_device
        holder["extractor"] = "discriminator" if args.fd_extractor == "discriminator" else \
            inception_features_device(args.fd_extractor, device)
    return holder["extractor"]


def _sampled(args, name, ds, losses, device, holder):
    """(real, extractor, what every sampling metric's constructor takes) of --<name>_samples: ``metric_inputs`` by flag name"""
    real, extractor, noise, batch = metric_inputs(args, getattr(args, name + "_samples"), "--%s_samples" % name, ds, losses, device,
                                                  holder)
    return real, extractor, dict(noise=noise, seed=args.seed, batch_size=batch)


def build_fd_metric(args, ds, losses, device, holder):
    """--fd_samples: the Frechet-distance metric over the first N items of ``ds`` (metric_inputs)."""
    from rna_gan_amd.metrics import FrechetDistance
    real, extractor, common = _sampled(args, "fd", ds, losses, device, holder)
    return FrechetDistance(real, extractor=extractor, **common)


def build_kid_metric(args, ds, losses, device, holder):
    """--kid_samples: the kernel-distance metric over the first N items of ``ds`` (metric_inputs: with --fd_samples N the same
    device copy of the real set and the same noise callable as the Frechet distance's)."""
    from rna_gan_amd.metrics import KernelDistance
    real, extractor, common = _sampled(args, "kid", ds, losses, device, holder)
    return KernelDistance(real, extractor=extractor, num_subsets=args.kid_subsets, subset_size=args.kid_subset_size, **common)


def build_qc_metric(args, ds, losses, device, holder):
    """--qc_samples: the tissue yield of N generated tiles.  The metric judges no real tile; metric_inputs supplies the noise
    (wganvae: built from the RNA rows of the first N items, shared with the other metrics over N samples) and the number of
    readable items, which is the number of generated tiles."""
    from rna_gan_amd.metrics import TissueYield
    real, _extractor, common = _sampled(args, "qc", ds, losses, device, holder)
    return TissueYield(int(real.shape[0]), **common)


def build_div_metric(args, ds, losses, device, holder):
    """--div_samples: the mean MS-SSIM over random pairs of N generated tiles.  metric_inputs supplies the noise (shared with the
    other metrics over N samples) and the first N readable items, which -- turned back to the bytes they were decoded from by
    ``export.tiles_u8`` -- are the real baseline the same pair list is evaluated over."""
    from rna_gan_amd.export import tiles_u8
    from rna_gan_amd.metrics import PairDiversity
    real, _extractor, common = _sampled(args, "div", ds, losses, device, holder)
    return PairDiversity(int(real.shape[0]), pairs=args.div_pairs or None, real=tiles_u8(real.float().contiguous()), **common)


def build_mem_metric(args, ds, losses, device, holder):
    """--mem_samples: the memorisation audit of N generated tiles.  Built without training tiles -- the resident set does not exist
    yet; main() hands it over with ``set_train`` -- and with metric_inputs' noise, as the tissue yield (wganvae: from the RNA rows of
    the first N items, shared with the other metrics over N samples)."""
    from rna_gan_amd.metrics import Memorisation
    real, _extractor, common = _sampled(args, "mem", ds, losses, device, holder)
    return Memorisation(None, int(real.shape[0]), factor=args.mem_factor, d4=bool(args.mem_d4), **common)


def build_pr_metric(args, ds, losses, device, holder):
    """--pr_samples: precision / recall / density / coverage over the first N items of ``ds`` (metric_inputs: with --fd_samples N
    or --kid_samples N the same device copy of the real set, the same noise callable and the same extractor)."""
    from rna_gan_amd.metrics import PrecisionRecall
    real, extractor, common = _sampled(args, "pr", ds, losses, device, holder)
    if real.shape[0] < args.pr_k + 1:
        raise SystemExit("--pr_samples: %d readable tiles among the first %d items, --pr_k %d needs %d"
                         % (real.shape[0], args.pr_samples, args.pr_k, args.pr_k + 1))
    return PrecisionRecall(real, extractor=extractor, nearest_k=args.pr_k, report=args.pr_report, **common)


def build_cf_metric(args, ds, losses, device, holder):
    """--cf_patients: the conditioning fidelity over the first P distinct RNA rows of ``ds`` -- distinct by the bytes of the fp32
    row, the rule of DeviceTileSet.from_dataset -- each with its first --cf_tiles readable tiles (held on the device; uint8 under
    --device_transform / --resident, normalised on the device as the training batches are).  The extractor is the shared one."""
    from rna_gan_amd.metrics import ConditioningFidelity
    P_, T = args.cf_patients, args.cf_tiles
    rows, row_index, tiles, patient_of, have = [], {}, [], [], []
    known = getattr(ds, "rna_data_arrays", None)           # a PatchRNADataset: the rows without decoding a tile
    for i in range(len(ds)):
        if len(rows) == P_ and min(have) >= T:
            break
        item = None
        row = known[i] if known is not None else None
        if row is None:
            item = ds[i]
            row = item["rna_data"]
        key = row.to(torch.float32).contiguous().numpy().tobytes()
        p = row_index.get(key)
        if p is None:
            if len(rows) == P_:
                continue
            p = row_index[key] = len(rows)
            rows.append(row.to(torch.float32))
            have.append(0)
        if have[p] >= T:
            continue
        image = (item if item is not None else ds[i])["image"]
        if image is None:
            continue
        tiles.append(image)
        patient_of.append(p)
        have[p] += 1
    if len(rows) < 2 or min(have) < 1:
        raise SystemExit("--cf_patients: %d distinct RNA rows among %d items, %d of them without a readable tile"
                         % (len(rows), len(ds), sum(1 for h in have if h < 1)))
    return ConditioningFidelity(torch.stack(tiles).to(device), torch.tensor(patient_of, dtype=torch.int32), torch.stack(rows),
                                losses[0].betavae, tiles_per_patient=T, extractor=shared_extractor(args, device, holder),
                                seed=args.seed, batch_size=256, report=args.cf_report)


# (what switches it on, what builds it): the per-epoch metrics in the order they are evaluated and logged
METRIC_BUILDERS = (("fd_samples", build_fd_metric), ("kid_samples", build_kid_metric), ("pr_samples", build_pr_metric),
                   ("qc_samples", build_qc_metric), ("div_samples", build_div_metric), ("cf_patients", build_cf_metric),
                   ("mem_samples", build_mem_metric))


def main():
    args = parse_args()
    if args.precision not in ("bf16", "fp32", "fp16"):
        raise SystemExit("--precision must be bf16, fp16 or fp32")
    if args.loss_scaling not in ("static", "dynamic"):
        raise SystemExit("--loss_scaling must be static or dynamic")
    if args.loss_scaling == "dynamic" and args.precision != "fp16":
        raise SystemExit("--loss_scaling dynamic applies to --precision fp16 only")

    D_.set_sync_stats(bool(args.sync_stats))
    D_.init_from_env()
    # every rank builds its replicas (G, D, and -- without a checkpoint file -- the betaVAE copies inside the three
    # loss plugins) from the SAME seed; the per-rank offset is applied after construction, for noise / eps / data only
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    with open(args.config) as f:
        config = json.load(f)
    if D_.rank() == 0:
        print(10 * "-"); print("Config for this experiment \n"); print(config); print(10 * "-")
    args.flag = config.get("flag", "train_{date:%Y-%m-%d %H:%M:%S}".format(date=datetime.datetime.now()))
    img_size = config["img_size"]
    rna_features = config.get("rna_features", 19198)
    with_rna = args.loss_type == "wganvae"
    input_transform = None
    if args.device_transform or args.augment != "none" or args.resident:
        from rna_gan_amd.augment import InputTransform
        input_transform = InputTransform(0.5, 0.5, augment=args.augment, seed=args.seed, rank=D_.rank())
    if args.synthetic:
        ds = SyntheticTiles(args.steps_per_epoch * args.batch_size, img_size, rna_features, with_rna,
                            args.seed + 1000 * D_.rank(), as_u8=bool(args.device_transform or args.resident))
        shard = None                                       # (every rank draws a set of its own: the whole of it is its shard)
        if not args.resident:
            loader = DataLoader(ds, batch_size=args.batch_size, num_workers=0, pin_memory=True, drop_last=True)
    else:
        # the reference's data path (src/histopathology_gan.py:111-168): slide tables -> [log + StandardScaler on the
        # rna_ columns] -> per-slide tile sampling from the slide databases -> batches; rna_gan_amd.data restates the
        # record format / sampling / preparation (LMDB files need the `lmdb` package, directory stores do not)
        from rna_gan_amd import data as PD
        from rna_gan_amd.gan_utils import training_dataset
        # every rank must build the SAME tile list (the datasets draw their per-slide tile sample from the global `random`
        # generator, src/read_data.py:313-316, seeded here), so that the strided shards below partition one list
        # transforms None: uint8 tiles, normalised on the device
        ds = training_dataset(config, args.seed, args.num_patches, with_rna,
                              None if args.device_transform or args.resident else PD.ToFloatNormalize(0.5, 0.5))

        world = D_.world_size()
        collate_fn = make_collate_fn(with_rna, world)
        shard = shard_indices(len(ds), D_.rank(), world, args.batch_size) if world > 1 else None
        if not args.resident:
            if world > 1:
                # one shard of the (identical) tile list per rank, the SAME number of full batches on every rank: each train_op
                # issues a gradient all-reduce, so a rank with one batch more would pair its collectives with nobody
                ds = torch.utils.data.Subset(ds, shard)
            loader = DataLoader(ds, batch_size=args.batch_size, num_workers=4, pin_memory=True, collate_fn=collate_fn,
                                drop_last=world > 1)   # :163-168

    if args.gan_type not in ("dcgan", "dcgan_up"):
        raise SystemExit("--gan_type dcgan (the reference CLI's path) or dcgan_up (src/dcgan.py's DCGANUpGenerator, "
                         "which the reference defines but never selects); condgan/biggan/sagan sources are absent upstream")
    gan_network = {
        "generator": {"name": P.DCGANUpGenerator if args.gan_type == "dcgan_up" else P.DCGANGenerator,
                      "args": {"encoding_dims": 2048, "out_channels": 3, "step_channels": 64, "out_size": img_size,
                               "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.Tanh()},
                      "optimizer": {"name": Adam, "args": {"lr": 0.0001, "betas": (0.5, 0.999)}}},
        "discriminator": {"name": P.DCGANDiscriminator,
                          "args": {"in_size": img_size, "in_channels": 3, "step_channels": 64,
                                   "batchnorm": bool(args.critic_batchnorm), "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.LeakyReLU(0.2)},
                          "optimizer": {"name": Adam, "args": {"lr": 0.0004, "betas": (0.5, 0.999)}}},
    }
    if args.loss_type == "wgan":
        losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(clip=(-0.01, 0.01)),
                  P.WassersteinGradientPenalty()]
    elif args.loss_type == "wganvae":
        ck = args.betavae_checkpoint if os.path.exists(args.betavae_checkpoint) else None
        if ck is None and D_.rank() == 0:
            print("betaVAE checkpoint not found: using randomly initialised encoder weights")
        losses = [P.WassersteinGeneratorLossVAE(checkpoint=ck, rna_features=rna_features),
                  P.WassersteinDiscriminatorLossVAE(checkpoint=ck, rna_features=rna_features),
                  P.WassersteinGradientPenaltyVAE(checkpoint=ck, rna_features=rna_features)]
    else:
        raise SystemExit(f"Loss type {args.loss_type} not implemented on this path. Choose wgan or wganvae.")

    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("RNAGAN_DIST_BACKEND") == "gloo":
        local %= max(torch.cuda.device_count(), 1)       # functional multi-rank runs on fewer devices than ranks (dist.init_from_env)
    device = torch.device("cuda", local)
    epochs = args.num_epochs if args.num_epochs is not None else 5
    print("Device: {}".format(device)); print("Epochs: {}".format(epochs))
    holder = {"input_transform": input_transform}
    built = {flag: build(args, ds, losses, device, holder)  # the per-epoch metrics are evaluated by rank 0 alone
             for flag, build in METRIC_BUILDERS if D_.rank() == 0 and getattr(args, flag) > 0}
    metrics = list(built.values()) or None
    trainer = P.Trainer(gan_network, losses, metrics_list=metrics, checkpoints=args.model_dir, sample_size=64, epochs=epochs, devices=[0],
                        recon=args.image_dir, device=device, precision=args.precision, loss_scaling=args.loss_scaling,
                        ema_decay=args.g_ema if args.g_ema > 0.0 else None, ema_warmup=bool(args.g_ema_warmup),
                        input_transform=None if args.resident else input_transform)   # resident: the loader's transform
    holder["trainer"] = trainer
    if args.resident:
        # the rank's shard, read once and kept on the device; the evaluation sets above keep their own path (the first N items
        # of ds, normalised by the same transform without a draw)
        from rna_gan_amd.resident import DeviceTileLoader, DeviceTileSet
        tiles = DeviceTileSet.from_dataset(ds, device, items=shard, workers=0 if args.synthetic else 4,
                                           max_bytes=int(args.resident_max_gb * (1 << 30)) if args.resident_max_gb > 0 else None)
        print("Resident set on {}: {} tiles, {} bytes, {} unreadable records dropped, built in {:.1f} s".format(
            device, len(tiles), tiles.nbytes, tiles.dropped, tiles.build_seconds))
        loader = DeviceTileLoader(tiles, args.batch_size, transform=input_transform, seed=args.seed, rank=D_.rank())
        if len(loader) == 0:
            raise SystemExit("--resident 1: %d readable tiles do not fill one batch of %d" % (len(tiles), args.batch_size))
        if "mem_samples" in built:                        # the audit searches the rank's resident tiles
            built["mem_samples"].set_train(tiles)
    if args.checkpoint is not None:
        trainer.load_model(load_path=args.checkpoint)
    for loss in losses:                                   # identical frozen encoders on every rank (rank 0's)
        bv = getattr(loss, "betavae", None)
        if bv is not None and D_.world_size() > 1:
            bv.to(device)
            before = bv.signature()                       # which of this rank's three encoders held the same weights
            for t in list(bv.parameters()) + list(bv.buffers()):
                D_.broadcast_(t.data, 0)
            bv.weights_changed()
            # every rank runs the same construction, so encoders that shared weights before the broadcast (one checkpoint
            # file) share rank 0's afterwards: keep that identity for the per-batch latent cache (losses._LatentCache)
            bv.adopt_weights_token(("broadcast",) + tuple(before))
    torch.manual_seed(args.seed + D_.rank())
    np.random.seed(args.seed + D_.rank())
    trainer(loader)
    D_.flush()                     # data parallel: apply a trailing optimizer step before the process group goes away
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
