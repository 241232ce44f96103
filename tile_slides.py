#!/usr/bin/env python3
"""Tile slide rasters into tile stores: the counterpart of the reference's src/preprocess/patch_gen_grid.py, with the raster on the
device (rna_gan_amd.tiler).

    python tile_slides.py --wsi_path SLIDES --patch_path TILES --mask_path MASKS [--patch_size 768] [--max_patches_per_slide 2000]
                          [--dezoom_factor 1.0]

A "slide" is a raster FILE in --wsi_path: a ``.npy`` holding uint8 (H, W, 3) R, G, B (opened memory-mapped and uploaded in strips),
or an image Pillow opens.  A reader for scanner formats (.svs) is out of scope, and so is a raster that does not fit the device:
it is refused with a message, not streamed.  What the Aperio property told the reference comes from --app_mag (default 20) or from a
sidecar ``<slide file>.json`` with {"app_mag": 40}; the window read at level 0 is int(app_mag / 20 * dezoom_factor * patch_size)
pixels and is resized to patch_size exactly as PIL.Image.resize does.

Per slide (its id is the file name up to its second dot, as in the reference):
  --mask_path/<id>/mask.npy   the closed tissue mask, rows = y; REUSED when present.  It is made from the thumbnail
                              ``<slide file without extension><--thumbnail_suffix>`` (.npy or an image: a lower level of the
                              slide's own pyramid) when that flag is given and the file exists, else from a box thumbnail of
                              --thumb_factor (32).
  --patch_path/<id>/<id with .svs replaced by .db>/   a directory store in the reference's tile-record format: what
                              rna_gan_amd.data.open_tile_store reads and where PatchDataset(patch_data_path=--patch_path) looks for
                              the slide named <id> (--out_format store, the only format).
                              A slide whose --patch_path/<id> exists is SKIPPED, as in the reference.
  --qc_report                 also writes --patch_path/<id>/qc.csv: origin and acceptance statistics of every stored tile.
  --stain_norm macenko        the slide's accepted tiles are fitted together as one set (rna_gan_amd.stain: Macenko's method on
                              integer tables) and normalised on the device to --stain_target (``reference``, or a JSON file: a
                              StainFit, or the stain.json of an earlier run -- a cohort can be normalised to one of its own slides)
                              before they are stored; --patch_path/<id>/stain.json holds the fit and the target.  Acceptance and
                              qc.csv keep judging the raw windows.  A slide that cannot be fitted is stored unnormalised, with a
                              message and "normalized": false in stain.json.  Default none: every byte as before.
--synthetic tiles --synthetic_slides seeded rasters of --synthetic_size (rna_gan_amd.tiler.synthetic_slide) named
synthetic_<k>.svs instead of reading --wsi_path.  --num_process is accepted for the reference's command lines and ignored: one
process drives one device.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REFERENCE_FLAGS = [
    ("--wsi_path", str, None, "directory of slide rasters (.npy or images)"),
    ("--patch_path", str, None, "output directory of the tile stores"),
    ("--mask_path", str, None, "directory of the numpy masks"),
    ("--patch_size", int, 768, "tile edge, default 768"),
    ("--max_patches_per_slide", int, 2000, "stop after this many accepted tiles"),
    ("--num_process", int, 10, "accepted and ignored"),
    ("--dezoom_factor", float, 1.0, "1.0: tiles at 20x magnification, 2.0: at 10x"),
]
EXTRA_FLAGS = [
    ("--app_mag", float, 20.0, "magnification of the raster's level 0 (the Aperio property); a sidecar <slide file>.json overrides it"),
    ("--thumbnail_suffix", str, None, "suffix of a supplied thumbnail file beside each slide, e.g. _thumb.npy"),
    ("--thumb_factor", int, 32, "box thumbnail factor when no thumbnail is supplied (1..64)"),
    ("--batch", int, 256, "candidate windows per acceptance batch"),
    ("--min_tissue", float, 0.2, "the dilated tissue mask must cover MORE than this fraction of a window"),
    ("--out_format", str, "store", "store: a directory store in the reference's record format"),
    ("--synthetic_slides", int, 2, "--synthetic: number of rasters"),
    ("--synthetic_size", str, "2048x2560", "--synthetic: rows x columns of each raster"),
    ("--seed", int, 0, "--synthetic: seed of the first raster"),
    ("--device", int, 0, "device index"),
    ("--stain_norm", str, "none", "none, or macenko: fit each slide's accepted tiles together and normalise them on the device"),
    ("--stain_target", str, "reference", "reference (the published Macenko target), or a JSON file holding a StainFit or an earlier run's stain.json"),
]
IMAGE_SUFFIXES = (".png", ".tif", ".tiff", ".jpg", ".jpeg", ".bmp")
QC_COLUMNS = ("slide", "tile", "x", "y", "otsu_r", "otsu_g", "otsu_b", "otsu_s", "tissue_fraction", "luma_p1", "luma_p99")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Tile slide rasters into tile stores (MI355X path)")
    for flag, typ, default, text in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(flag, type=typ, default=default, help=text)
    ap.add_argument("--qc_report", action="store_true", help="write qc.csv per slide")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic rasters instead of --wsi_path")
    args = ap.parse_args(argv)
    if not args.patch_path or not args.mask_path:
        ap.error("--patch_path and --mask_path are required")
    if not args.synthetic and not args.wsi_path:
        ap.error("--wsi_path is required without --synthetic")
    if not 1 <= args.patch_size <= 1024:
        ap.error("--patch_size must be in 1..1024")
    if args.max_patches_per_slide < 0 or args.batch < 1:
        ap.error("--max_patches_per_slide must be >= 0 and --batch >= 1")
    if not args.dezoom_factor > 0 or not args.app_mag > 0:
        ap.error("--dezoom_factor and --app_mag must be positive")
    if not 1 <= args.thumb_factor <= 64:
        ap.error("--thumb_factor must be in 1..64")
    if not 0.0 <= args.min_tissue <= 1.0:
        ap.error("--min_tissue must be in [0, 1]")
    if args.out_format != "store":
        ap.error("--out_format must be store")
    if args.stain_norm not in ("none", "macenko"):
        ap.error("--stain_norm must be none or macenko")
    if args.stain_target != "reference" and args.stain_norm == "none":
        ap.error("--stain_target needs --stain_norm macenko")
    if args.stain_target != "reference" and not os.path.isfile(args.stain_target):
        ap.error("--stain_target must be reference or an existing JSON file")
    try:
        rows, cols = (int(v) for v in args.synthetic_size.lower().split("x"))
        if rows < 1 or cols < 1:
            raise ValueError
        args.synthetic_shape = (rows, cols)
    except ValueError:
        ap.error("--synthetic_size must be ROWSxCOLUMNS")
    if args.synthetic and args.synthetic_slides < 1:
        ap.error("--synthetic_slides must be >= 1")
    return args


def slide_id(name):
    """the reference's get_slide_id: the file name up to its second dot"""
    parts = name.split(".")
    return parts[0] + "." + parts[1] if len(parts) > 1 else parts[0]


def _open_raster(path):
    """a uint8 (H, W, 3) array: a memory map for .npy, else the decoded image"""
    if path.lower().endswith(".npy"):
        a = np.load(path, mmap_mode="r")
    else:
        from PIL import Image
        Image.MAX_IMAGE_PIXELS = None
        a = np.asarray(Image.open(path).convert("RGB"))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise SystemExit("%s: a slide raster is uint8 (H, W, 3), got %s %s" % (path, a.dtype, a.shape))
    return a


def list_slides(args):
    """[(slide id, slide file or seed, app_mag)]"""
    if args.synthetic:
        return [("synthetic_%d.svs" % k, args.seed + k, args.app_mag) for k in range(args.synthetic_slides)]
    out = []
    for name in sorted(os.listdir(args.wsi_path)):
        low = name.lower()
        if not (low.endswith(".npy") or low.endswith(IMAGE_SUFFIXES)):
            continue
        if args.thumbnail_suffix and name.endswith(args.thumbnail_suffix):
            continue
        path = os.path.join(args.wsi_path, name)
        mag = args.app_mag
        if os.path.exists(path + ".json"):
            with open(path + ".json") as f:
                side = json.load(f)
            mag = float(side.get("app_mag", side.get("aperio.AppMag", mag)))
        out.append((slide_id(name), path, mag))
    return out


def upload(a, device, working_bytes):
    """the raster on the device, copied in strips of rows; refused when it does not fit"""
    need = a.shape[0] * a.shape[1] * 3 + working_bytes
    free, _ = torch.cuda.mem_get_info(device)
    if need > free:
        raise SystemExit("a raster of %d x %d pixels needs %.1f GB on the device with its working buffers, %.1f GB are free: "
                         "a raster that does not fit is not streamed in strips (out of scope)" % (a.shape[0], a.shape[1], need / 1e9, free / 1e9))
    dst = torch.empty(a.shape, dtype=torch.uint8, device=device)
    rows = max(1, (256 << 20) // (a.shape[1] * 3))
    for r in range(0, a.shape[0], rows):
        dst[r:r + rows].copy_(torch.from_numpy(np.ascontiguousarray(a[r:r + rows])))
    return dst


def run(args):
    """The work of the CLI.  Returns the list of paths written."""
    from rna_gan_amd import tiler, tissue
    from rna_gan_amd.data import write_tile_store
    device = torch.device("cuda", args.device)
    torch.cuda.set_device(device)
    written = []
    if args.stain_norm == "macenko":
        from rna_gan_amd import stain
        target = stain.load_target(args.stain_target)
    for sid, src, mag in list_slides(args):
        folder = os.path.join(args.patch_path, sid)
        if os.path.isdir(folder):
            print("slide %s: %s exists, skipped" % (sid, folder))
            continue
        a = tiler.synthetic_slide(args.synthetic_shape[0], args.synthetic_shape[1], seed=src) if args.synthetic else _open_raster(src)
        read = int(mag / 20.0 * args.dezoom_factor * args.patch_size)
        if read < 1 or read > tiler.MAX_READ:
            raise SystemExit("slide %s: the window at level 0 would be %d pixels (1..%d)" % (sid, read, tiler.MAX_READ))
        working = args.batch * (3 * read * read + 3 * args.patch_size ** 2 + read * read + (64 << 10)) + (a.shape[0] * a.shape[1]) // 8
        raster = upload(a, device, working)
        os.makedirs(folder)
        mask_file = os.path.join(args.mask_path, sid, "mask.npy")
        mask = thumb = None
        if os.path.exists(mask_file):
            mask = torch.from_numpy(np.load(mask_file).astype(np.uint8))
        elif args.thumbnail_suffix and not args.synthetic:
            t = os.path.splitext(src)[0] + args.thumbnail_suffix
            if os.path.exists(t):
                thumb = torch.from_numpy(np.ascontiguousarray(_open_raster(t)))
        res = tiler.tile_raster(raster, thumbnail=thumb, patch_size=args.patch_size, app_mag=mag, dezoom=args.dezoom_factor,
                                max_patches=args.max_patches_per_slide, batch=args.batch, thumb_factor=args.thumb_factor,
                                min_tissue=args.min_tissue, order="rgb", mask=mask)
        if mask is None:
            os.makedirs(os.path.dirname(mask_file), exist_ok=True)
            np.save(mask_file, res.mask.cpu().numpy().astype(bool))
            written.append(mask_file)
        tiles = res.tiles
        if args.stain_norm == "macenko":                 # the acceptance rule and qc.csv have judged the raw windows
            fitted, message = None, None
            try:
                fitted = stain.fit(tiles, layout="nhwc", order="rgb", batch=args.batch)
                tiles = stain.normalize(tiles, fitted, target)
            except stain.StainFitError as e:
                message = str(e)
                print("slide %s: not stain-normalised, stored as tiled: %s" % (sid, message))
            path = os.path.join(folder, "stain.json")
            with open(path, "w") as f:
                f.write(stain.stain_report(fitted, target, message is None, message))
            written.append(path)
        tiles = tiles.cpu().numpy()
        path = os.path.join(folder, sid.replace(".svs", ".db"))
        write_tile_store(path, tiles, slide_id=sid, stored=True, channel_order="rgb")
        written.append(path)
        if args.qc_report:
            st = tissue.stats_from_rows(res.qc, res.read, res.read)
            frac, pct = tissue.tissue_fraction(st), tissue.luma_percentiles(st)
            path = os.path.join(folder, "qc.csv")
            with open(path, "w") as f:
                f.write(",".join(QC_COLUMNS) + "\n")
                for k in range(len(res)):
                    row = res.qc[k]
                    f.write("%s,%d,%d,%d,%d,%d,%d,%d,%r,%r,%r\n" % (sid, k, res.origins[k, 0], res.origins[k, 1], row[0], row[1], row[2],
                                                                   row[3], float(frac[k]), float(pct[k, 0]), float(pct[k, 1])))
            written.append(path)
        if len(res) == 0:
            print("no patch extracted for slide %s" % sid)
        print("slide %s: %d x %d, read %d -> %d, %d candidates, %d in the mask, %d examined, %d tiles" % (
            sid, a.shape[0], a.shape[1], res.read, args.patch_size, res.candidates, res.in_mask, res.examined, len(res)))
        del raster, res
    return written


def main(argv=None):
    args = parse_args(argv)
    written = run(args)
    print(json.dumps({"written": written}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
