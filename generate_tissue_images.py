#!/usr/bin/env python3
"""Working counterpart of the reference's generation CLI (src/generate_tissue_images.py) on the MI355X path: tiles from gene
expression.

The reference flag set (--config --checkpoint --checkpoint2 --patient1 --sample_size --rna_features --rna_file --vae_checkpoint
--save_path --random_patient) is kept.  The reference script itself cannot run (it reads ``args.vae`` and ``args.save_dir``,
which it never defines, and needs cv2 and matplotlib); two modes work here:

  --random_patient   one row of --rna_file (the columns whose name contains ``rna_``, values as they are) conditions
                     --sample_size tiles; ONE 8 x 8 grid PNG goes to --save_path.  The grid is composed on the host from the
                     uint8 tiles (numpy + PIL).
  bulk               --patients all|<comma list of row numbers or of values of --id_column> --tiles_per_patient N --out_dir D
                     --out_format store|png|npy:
                       store  one directory store per patient, D/<id>/<id with .svs replaced by .db>/, in the reference's
                              tile-record format (stored LZ4 blocks): what rna_gan_amd.data.open_tile_store reads and where
                              PatchDataset(patch_data_path=D) looks for the slide named <id>
                       png    D/<id>/<t>.png          npy    D/<id>.npy, one (N, H, W, 3) uint8 array per patient
Both run through rna_gan_amd.gan_utils.generate_tiles: the tiles are quantised and interleaved on the device
(rg_tile_export_u8) and cross the host link as uint8 behind a double-buffered pinned download.

--qc report|filter (bulk mode) holds the generated tiles to the acceptance rule of the reference's tiler (rna_gan_amd.tissue: the
tissue mask, dilated --qc_dilate times, covers more than --qc_min_tissue of the tile and the tile is not low-contrast).  The rule runs on the uint8
chunk where it lies on the device; 12 integers per tile travel with the chunk.  report writes D/qc.csv (one row per tile: patient,
tile, stored_index, the four Otsu thresholds, tissue_fraction, the two luma percentiles, low_contrast, accepted); filter also
leaves the rejected tiles out of the output (the kept ones are renumbered in tile order; stored_index names them, -1 = left out)
and prints how many per patient.  off (the default) runs none of it: every output byte is as without the flag.

Extra flags: --prepare_rna 1 (log_standardize_rna over the file's rows first), --quantize round|trunc (trunc reproduces the
reference script's ``img *= 255; astype(uint8)``; round returns a tile that went through the input transform unchanged),
--g_ema 1 (the checkpoint's averaged generator), --fp8 1, --chunk, --group, --seed, --precision; --synthetic runs on seeded random
weights and synthetic RNA rows instead of the three files, like every other CLI here.

With ONE patient every row of a standardisation group carries the same encoder output, and the column standardisation removes
it: the tiles are conditioned on the uniform draw alone.  The reference's generate_images behaves the same; a warning is printed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REFERENCE_FLAGS = [
    ("--config", str, None, "JSON config file (optional here: rna_features / img_size are read from it when present)"),
    ("--checkpoint", str, None, "generator checkpoint (a Trainer .model file)"),
    ("--checkpoint2", str, None, "accepted for the reference's command lines; the unconditioned second model is not used"),
    ("--patient1", str, None, "patient id: a value of --id_column (bulk mode: the same as --patients <id>)"),
    ("--sample_size", int, 64, "tiles of the --random_patient grid"),
    ("--rna_features", int, 19198, "number of genes"),
    ("--rna_file", str, None, "CSV with the gene expression (columns whose name contains rna_)"),
    ("--vae_checkpoint", str, None, "betaVAE state dict"),
    ("--save_path", str, None, "--random_patient: file name of the grid PNG"),
]
EXTRA_FLAGS = [
    ("--patients", str, None, "bulk mode: all, or a comma list of row numbers or of values of --id_column"),
    ("--id_column", str, None, "column of --rna_file that names the patients (default: row numbers)"),
    ("--tiles_per_patient", int, 0, "bulk mode: tiles per patient"),
    ("--out_dir", str, None, "bulk mode: output directory"),
    ("--out_format", str, "store", "bulk mode: store, png or npy"),
    ("--prepare_rna", int, 0, "1 = natural log + StandardScaler over the file's rows first (log_standardize_rna)"),
    ("--quantize", str, "round", "round (v * 255 + 0.5) or trunc (v * 255, the reference script's rule)"),
    ("--g_ema", int, 0, "1 = the checkpoint's averaged generator (generator_ema)"),
    ("--fp8", int, 0, "1 = fp8 e4m3 on the generator layers that have an fp8 kernel"),
    ("--chunk", int, 512, "tiles per generator launch sequence and per download"),
    ("--group", int, 4096, "rows per column standardisation"),
    ("--seed", int, 0, "seed of the private uniform draw (and of --random_patient's row choice)"),
    ("--precision", str, "bf16", "bf16, fp16 or fp32"),
    ("--img_size", int, 256, "--synthetic: tile edge"),
    ("--qc", str, "off", "bulk mode: off, report (write qc.csv beside the output) or filter (also leave rejected tiles out)"),
    ("--qc_min_tissue", float, 0.2, "--qc: the dilated tissue mask must cover MORE than this fraction of a tile"),
    ("--qc_dilate", int, 3, "--qc: iterations of the 4-connected dilation of the tissue mask (0..8; the reference tiler's 3)"),
    ("--qc_rgb_min", int, 50, "--qc: a tissue pixel has R, G and B above this (0..255; the reference tiler's 50)"),
]
QC_COLUMNS = ("patient", "tile", "stored_index", "otsu_r", "otsu_g", "otsu_b", "otsu_s", "tissue_fraction", "luma_p1", "luma_p99",
              "low_contrast", "accepted")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Generate tiles from gene expression (MI355X path)")
    for flag, typ, default, text in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(flag, type=typ, default=default, help=text)
    ap.add_argument("--random_patient", action="store_true", default=False, help="one random row of --rna_file, one 8 x 8 grid")
    ap.add_argument("--synthetic", action="store_true", help="seeded random weights and synthetic RNA rows instead of the files")
    args = ap.parse_args(argv)
    if args.patient1 is not None and args.patients is None:
        args.patients = args.patient1
    bulk = args.patients is not None
    if args.random_patient and bulk:
        ap.error("--random_patient and --patients / --patient1 exclude each other")
    if not args.random_patient and not bulk:
        ap.error("choose --random_patient or bulk mode (--patients all|<list>)")
    if args.random_patient:
        if not args.save_path:
            ap.error("--random_patient needs --save_path")
        if not 2 <= args.sample_size <= 64:
            ap.error("--sample_size must be in 2..64 (one 8 x 8 grid; a column standardisation needs two rows)")
    else:
        if not args.out_dir:
            ap.error("bulk mode needs --out_dir")
        if args.tiles_per_patient < 1:
            ap.error("bulk mode needs --tiles_per_patient >= 1")
        if args.out_format not in ("store", "png", "npy"):
            ap.error("--out_format must be store, png or npy")
        if not args.patients.strip():
            ap.error("--patients must be all or a comma list")
    if args.qc not in ("off", "report", "filter"):
        ap.error("--qc must be off, report or filter")
    if args.qc != "off" and args.random_patient:
        ap.error("--qc belongs to bulk mode")
    if not 0.0 <= args.qc_min_tissue <= 1.0:
        ap.error("--qc_min_tissue must be in [0, 1]")
    if not 0 <= args.qc_dilate <= 8 or not 0 <= args.qc_rgb_min <= 255:
        ap.error("--qc_dilate must be in 0..8 and --qc_rgb_min in 0..255")
    if not args.synthetic:
        for flag in ("checkpoint", "rna_file", "vae_checkpoint"):
            if getattr(args, flag) is None:
                ap.error("--%s is required without --synthetic" % flag)
    if args.quantize not in ("round", "trunc"):
        ap.error("--quantize must be round or trunc")
    from rna_gan_amd.gan_utils import check_flags
    check_flags(ap, args, binary=("prepare_rna", "g_ema", "fp8"))
    if args.chunk < 1:
        ap.error("--chunk must be >= 1")
    if args.group < 2:
        ap.error("--group must be >= 2")
    if args.fp8 and args.precision != "bf16":
        ap.error("--fp8 1 needs --precision bf16")
    if args.rna_features < 1 or args.img_size < 1:
        ap.error("--rna_features and --img_size must be positive")
    return args


def load_rna(args):
    """(ids, rows): the patients' names and the (P_all, features) float32 expression rows of --rna_file / --synthetic."""
    if args.synthetic:
        from rna_gan_amd.synth import synthetic_rna
        rows = synthetic_rna(16, args.rna_features, seed=args.seed + 1, distinct=16)
        return [str(i) for i in range(rows.shape[0])], rows
    import pandas as pd
    df = pd.read_csv(args.rna_file)
    if args.prepare_rna:
        from rna_gan_amd.data import log_standardize_rna
        df = log_standardize_rna(df)[0]
    cols = [c for c in df.columns if "rna_" in c]
    if not cols:
        raise SystemExit("%s has no column whose name contains rna_" % args.rna_file)
    ids = [str(v) for v in df[args.id_column]] if args.id_column else [str(i) for i in range(len(df))]
    return ids, torch.from_numpy(df[cols].to_numpy(dtype=np.float32))


def select_patients(spec, ids):
    """Row numbers for ``all`` or a comma list of ids."""
    if spec == "all":
        return list(range(len(ids)))
    index = {}
    for i, v in enumerate(ids):
        index.setdefault(v, i)
    rows = []
    for tok in (t.strip() for t in spec.split(",")):
        if tok not in index:
            raise SystemExit("no patient %r in the RNA table" % tok)
        if index[tok] in rows:
            raise SystemExit("patient %r is listed twice" % tok)
        rows.append(index[tok])
    return rows


def compose_grid(tiles, rows=8, cols=8):
    """(n, H, W, 3) uint8, n <= rows * cols -> one (rows * H, cols * W, 3) uint8 image, row-major, unused cells black."""
    n, H, W, C = tiles.shape
    grid = np.zeros((rows * H, cols * W, C), dtype=np.uint8)
    for i in range(min(n, rows * cols)):
        r, q = divmod(i, cols)
        grid[r * H:(r + 1) * H, q * W:(q + 1) * W] = tiles[i]
    return grid


def run(args, trainer=None, betavae=None):
    """The work of the CLI.  trainer / betavae: models handed in (tests); otherwise built from the arguments.  Returns the
    list of paths written."""
    from PIL import Image
    from rna_gan_amd.data import write_tile_store
    from rna_gan_amd.gan_utils import build_models, generate_tiles
    if trainer is None or betavae is None:
        trainer, betavae = build_models(args, torch.device("cuda", 0), synthetic_betavae=True)
    ids, rows = load_rna(args)
    common = dict(seed=args.seed, ema=bool(args.g_ema), fp8=bool(args.fp8), chunk=args.chunk, group=args.group,
                  layout="nhwc", order="rgb", rounding=args.quantize)
    if args.random_patient:
        pick = int(np.random.default_rng(args.seed).integers(0, len(ids)))
        print("patient %s: one patient -- the column standardisation removes the encoder's output, the tiles are conditioned "
              "on the uniform draw alone (as in the reference's generate_images)" % ids[pick], file=sys.stderr)
        tiles = None
        for _p, t, a in generate_tiles(trainer, rows[pick:pick + 1], args.sample_size, betavae, **common):
            if tiles is None:
                tiles = np.empty((args.sample_size,) + a.shape[1:], dtype=np.uint8)
            tiles[t] = a
        d = os.path.dirname(args.save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        Image.fromarray(compose_grid(tiles)).save(args.save_path)
        return [args.save_path]
    sel = select_patients(args.patients, ids)
    if len(sel) == 1:
        print("WARNING: one patient -- the column standardisation over a group removes the encoder's output, so the tiles are "
              "conditioned on the uniform draw alone (the reference's generate_images behaves the same)", file=sys.stderr)
    T = args.tiles_per_patient
    os.makedirs(args.out_dir, exist_ok=True)
    names = [ids[i] for i in sel]
    written = []
    qc_on = args.qc != "off"
    qc_rows = {}                  # (patient, tile) -> (12 integers, tissue fraction, percentiles, low_contrast, accepted)
    # tile-major walk: a patient's tiles arrive spread over the whole run.  png files are written as they arrive; store and npy
    # collect one (T, H, W, 3) array per patient (3 bytes per pixel on the host)
    per_patient = {}
    qc = dict(dilate=args.qc_dilate, rgb_min=args.qc_rgb_min) if qc_on else None
    for item in generate_tiles(trainer, rows[sel], T, betavae, qc=qc, **common):
        p, t, a = item[0], item[1], item[2]
        keep = np.ones(a.shape[0], dtype=bool)
        if qc_on:
            from rna_gan_amd import tissue as TQ
            st = TQ.stats_from_rows(item[3], a.shape[1], a.shape[2], **qc)
            ok = TQ.accept(st, min_tissue=args.qc_min_tissue)
            frac, pct, low = TQ.tissue_fraction(st), TQ.luma_percentiles(st), TQ.low_contrast(st)
            for k in range(a.shape[0]):
                qc_rows[(int(p[k]), int(t[k]))] = (st.stats[k].copy(), float(frac[k]), pct[k].copy(), bool(low[k]), bool(ok[k]))
            if args.qc == "filter":
                keep = ok
        if args.out_format == "png":
            for k in range(a.shape[0]):
                if not keep[k]:
                    continue
                d = os.path.join(args.out_dir, names[p[k]])
                os.makedirs(d, exist_ok=True)
                path = os.path.join(d, "%d.png" % t[k])
                Image.fromarray(a[k]).save(path)
                written.append(path)
        else:
            for q in np.unique(p):
                if q not in per_patient:
                    per_patient[q] = np.empty((T,) + a.shape[1:], dtype=np.uint8)
                m = p == q
                per_patient[q][t[m]] = a[m]
    stored_index = {}
    for q in range(len(sel)):
        kept = [t for t in range(T) if args.qc != "filter" or qc_rows[(q, t)][4]]
        # png files keep their tile number as their name; store and npy renumber what is kept
        stored_index.update({(q, t): (t if args.out_format == "png" else i) for i, t in enumerate(kept)})
        if args.qc == "filter":
            print("patient %s: %d of %d tiles rejected" % (names[q], T - len(kept), T))
            if q in per_patient:
                per_patient[q] = per_patient[q][kept]
    for q, tiles in sorted(per_patient.items()):
        if args.out_format == "store":
            # where PatchDataset(patch_data_path=out_dir) looks for the slide named <id> (rna_gan_amd/data.py)
            path = os.path.join(args.out_dir, names[q], names[q].replace(".svs", ".db"))
            write_tile_store(path, tiles, slide_id=names[q], stored=True, channel_order="rgb")
        else:
            path = os.path.join(args.out_dir, names[q] + ".npy")
            np.save(path, tiles)
        written.append(path)
    if qc_on:
        path = os.path.join(args.out_dir, "qc.csv")
        with open(path, "w") as f:
            f.write(",".join(QC_COLUMNS) + "\n")
            for (q, t) in sorted(qc_rows):
                row, frac, pct, low, ok = qc_rows[(q, t)]
                f.write("%s,%d,%d,%d,%d,%d,%d,%r,%r,%r,%d,%d\n" % (names[q], t, stored_index.get((q, t), -1), row[0], row[1], row[2],
                                                                  row[3], frac, float(pct[0]), float(pct[1]), low, ok))
        written.append(path)
    return written


def main(argv=None):
    args = parse_args(argv)
    if args.config:
        with open(args.config) as f:
            config = json.load(f)
        print(10 * "-"); print("Config for this experiment \n"); print(config); print(10 * "-")
        args.rna_features = int(config.get("rna_features", args.rna_features))
    for path in run(args)[:8]:
        print(path)


if __name__ == "__main__":
    main()
