#!/usr/bin/env python3
"""Stain-normalise tile stores that already exist (tile_slides.py's, or the reference tiler's): Macenko's method on the device
(rna_gan_amd.stain), one fit per slide over all its tiles.

    python stain_normalize.py --patch_path TILES --out_path NORMALISED [--stain_target reference|FILE.json] [--batch 256]

Per slide folder --patch_path/<id>/ with a store <name>.db (a directory store or an LMDB file, rna_gan_amd.data.open_tile_store):
read the tiles, fit them together, normalise them to the target and write --out_path/<id>/<name>.db as a directory store with the
same record names and channel order, and --out_path/<id>/stain.json (the fit and the target).  A slide whose output folder exists
is SKIPPED.  A slide that cannot be fitted (too few stained pixels, ...) is copied unnormalised with a printed message and
"normalized": false in stain.json.  --stain_target: ``reference`` (the published Macenko target) or a JSON file holding a StainFit
or an earlier run's stain.json, so that a cohort can be normalised to one of its own slides.
--synthetic first writes two small seeded stores into --patch_path (when it is empty or missing) so that the program can be tried
without data.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Macenko stain normalisation of tile stores (MI355X path)")
    ap.add_argument("--patch_path", type=str, default=None, help="directory of the slide folders to read")
    ap.add_argument("--out_path", type=str, default=None, help="directory of the normalised slide folders")
    ap.add_argument("--stain_target", type=str, default="reference", help="reference, or a JSON file holding a StainFit / a stain.json")
    ap.add_argument("--batch", type=int, default=256, help="tiles per accumulating launch of the fit")
    ap.add_argument("--synthetic", action="store_true", help="write two small seeded stores into --patch_path first")
    ap.add_argument("--device", type=int, default=0, help="device index")
    args = ap.parse_args(argv)
    if not args.patch_path or not args.out_path:
        ap.error("--patch_path and --out_path are required")
    if os.path.abspath(args.patch_path) == os.path.abspath(args.out_path):
        ap.error("--out_path must differ from --patch_path")
    if args.batch < 1:
        ap.error("--batch must be >= 1")
    if args.stain_target != "reference" and not os.path.isfile(args.stain_target):
        ap.error("--stain_target must be reference or an existing JSON file")
    if not args.synthetic and not os.path.isdir(args.patch_path):
        ap.error("--patch_path %s is not a directory" % args.patch_path)
    return args


def list_stores(patch_path):
    """[(slide id, store name, store path)]: every <patch_path>/<id>/<name>.db"""
    out = []
    for sid in sorted(os.listdir(patch_path)):
        folder = os.path.join(patch_path, sid)
        if not os.path.isdir(folder):
            continue
        for name in sorted(os.listdir(folder)):
            if name.endswith(".db"):
                out.append((sid, name, os.path.join(folder, name)))
    return out


def read_store(path):
    """(record names, tiles uint8 (n, H, W, 3) in the STORED channel order) of one store; None for a store without tiles"""
    from rna_gan_amd.data import lz4f_decompress, open_tile_store
    store = open_tile_store(path)
    keys = pickle.loads(lz4f_decompress(store[b"__keys__"]))
    names, tiles = [], []
    for k in keys:
        name, raw, shape = pickle.loads(lz4f_decompress(store[k]))
        names.append(name)
        tiles.append(np.frombuffer(raw, dtype=np.uint8).reshape(shape))
    if hasattr(store, "close"):
        store.close()
    if not tiles:
        return None
    if any(t.shape != tiles[0].shape for t in tiles) or tiles[0].ndim != 3 or tiles[0].shape[2] != 3:
        raise SystemExit("%s: the tiles of a store must share one (H, W, 3) shape" % path)
    return names, np.stack(tiles)


def write_store(path, names, tiles):
    """a directory store with the given record names; tiles in the stored channel order"""
    from rna_gan_amd.data import encode_keys, encode_record
    os.makedirs(path)
    for i, (name, tile) in enumerate(zip(names, tiles)):
        with open(os.path.join(path, str(i)), "wb") as f:
            f.write(encode_record(name, tile, stored=True))
    with open(os.path.join(path, "__keys__"), "wb") as f:
        f.write(encode_keys(len(names)))


def write_synthetic(patch_path, slides=2, tiles=6, size=64):
    """small seeded H&E-like stores (Beer-Lambert mixtures of two stains, a different pair per slide)"""
    from rna_gan_amd.data import write_tile_store
    stains = (((0.65, 0.70, 0.29), (0.07, 0.99, 0.11)), ((0.55, 0.76, 0.35), (0.21, 0.91, 0.36)))
    for k in range(slides):
        rng = np.random.default_rng(k)
        he = np.array(stains[k % 2], dtype=np.float64).T
        he /= np.linalg.norm(he, axis=0)
        conc = np.stack([rng.gamma(2.0, 0.45, tiles * size * size), rng.gamma(2.0, 0.3, tiles * size * size)], axis=1)
        conc[rng.random(conc.shape[0]) < 0.25] = 0.0
        img = 240.0 * np.exp(-(conc @ he.T)) + rng.normal(0.0, 1.5, (conc.shape[0], 3))
        rgb = np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(tiles, size, size, 3)
        sid = "synthetic_%d.svs" % k
        write_tile_store(os.path.join(patch_path, sid, sid.replace(".svs", ".db")), rgb, slide_id=sid, stored=True, channel_order="rgb")


def run(args):
    """The work of the CLI.  Returns the list of paths written."""
    from rna_gan_amd import stain
    device = torch.device("cuda", args.device)
    torch.cuda.set_device(device)
    target = stain.load_target(args.stain_target)
    if args.synthetic and not (os.path.isdir(args.patch_path) and os.listdir(args.patch_path)):
        write_synthetic(args.patch_path)
    written = []
    done = set()
    for sid, name, path in list_stores(args.patch_path):
        folder = os.path.join(args.out_path, sid)
        if sid not in done and os.path.isdir(folder):
            print("slide %s: %s exists, skipped" % (sid, folder))
            continue
        got = read_store(path)
        if got is None:
            print("slide %s: %s holds no tile, skipped" % (sid, name))
            continue
        names, tiles = got
        done.add(sid)
        dev = torch.from_numpy(tiles).to(device)
        fitted, message = None, None
        try:                                             # the records hold B, G, R (the reference's order)
            fitted = stain.fit(dev, layout="nhwc", order="bgr", batch=args.batch)
            dev = stain.normalize(dev, fitted, target, layout="nhwc", order="bgr")
        except stain.StainFitError as e:
            message = str(e)
            print("slide %s: not stain-normalised, copied as stored: %s" % (sid, message))
        out = os.path.join(folder, name)
        write_store(out, names, dev.cpu().numpy())
        written.append(out)
        report = os.path.join(folder, "stain.json")
        with open(report, "w") as f:
            f.write(stain.stain_report(fitted, target, message is None, message))
        written.append(report)
        print("slide %s: %d tiles of %d x %d%s" % (sid, len(names), tiles.shape[1], tiles.shape[2],
                                                   "" if fitted is None else ", %d of %d pixels stained" % (fitted.n_stained, fitted.n_pixels)))
    return written


def main(argv=None):
    args = parse_args(argv)
    written = run(args)
    print(json.dumps({"written": written}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
