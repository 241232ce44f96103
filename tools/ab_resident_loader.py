#!/usr/bin/env python3
"""The resident training set (rg_tile_gather_transform, rna_gan_amd.resident) measured on one device.

    python tools/ab_resident_loader.py [--batch 64 --size 256 --tiles 4096] [--json profiles/resident_loader.json]

Sections:
  build    the one-off cost: DeviceTileSet.from_dataset over --tiles synthetic uint8 tiles (histopathology_gan.SyntheticTiles,
           0 workers: the time is the host's numpy draw plus the chunked uploads), host clock ending in a device synchronise,
           and the bytes resident.  The kernel section gathers from this set.
  kernel   one batch [--batch][3][--size][--size] with mixed per-sample codes and a random index into the set, device events
           around --reps back-to-back calls, every variant timed once per round, the order reversed every other round, (g)
           timed twice per round (the difference of its two identically configured timings is the noise floor):
             (g) rg_tile_gather_transform: gather + normalise + D4 in one launch
             (t) the two-pass form it replaces: torch.index_select on the uint8 store, then rg_tile_transform
             (c) rg_tile_transform on a CONTIGUOUS batch of the store (the same bytes moved, no index)
           The calls rotate over --sets index sets / destinations; the set itself (--tiles x 196 608 B) and the destinations
           exceed the 256 MiB Infinity Cache.  Acceptance: (g) <= (t) beyond the noise floor; g / c is reported, not gated.
  train    Trainer.train iterations per second, reference-size networks, stock wgan plugins, one trainer per variant, a warm-up
           pass each, then --train_rounds interleaved timed passes of --steps iterations (host clock around a pass that ends in
           a device synchronise; checkpoints are not written):
             u8_loader       the in-process uint8 DataLoader + InputTransform (--device_transform 1)
             resident_none   DeviceTileLoader, no symmetry
             resident_d4     DeviceTileLoader, D4 codes
             fixed_batch     ONE final fp32 device batch handed out every iteration: the loop's rate with no input work at all
                             (what is left between a resident rate and this one is the loader's host code and index_select;
                             what is left between this one and the step's own rate is the Trainer's and the plugins' host code)
           Acceptance: resident_none and resident_d4 above u8_loader.
Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402


def event_us(fn, reps, device):
    """microseconds per call over `reps` back-to-back calls between two device events"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def interleave(variants, rounds, measure, tag):
    names = list(variants)
    out = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            out[n].append(measure(variants[n]))
        print("[ab_resident_loader] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)),
              file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


class FixedBatch:
    """Hands out the same final device batch `steps` times."""
    final_images = True

    def __init__(self, batch, steps):
        self.batch, self.steps, self.batch_size = batch, steps, batch[0].shape[0]

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield list(self.batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tiles", type=int, default=4096, help="tiles of the resident set (build and kernel sections)")
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--train_rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out (kernel needs build)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    import histopathology_gan as H
    from rna_gan_amd import _abi
    from rna_gan_amd.resident import DeviceTileLoader, DeviceTileSet
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    N, S, M = a.batch, a.size, a.tiles
    res = {"what": "resident training set on one device; variants interleaved in one process", "batch": N, "size": S,
           "device": torch.cuda.get_device_name(device)}

    ts = None
    if "build" not in skip:
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        ts = DeviceTileSet.from_dataset(H.SyntheticTiles(M, S, 8, False, 7, as_u8=True), device)
        torch.cuda.synchronize(device)
        res["build"] = {"tiles": len(ts), "seconds": round(time.perf_counter() - t0, 2), "bytes_resident": ts.nbytes,
                        "dropped": ts.dropped, "source": "histopathology_gan.SyntheticTiles as_u8, 0 workers, chunks of 256: the "
                        "host's numpy draw of every tile plus the pinned uploads"}
        print("[ab_resident_loader] build: %s" % json.dumps(res["build"]), file=sys.stderr, flush=True)

    if "kernel" not in skip:
        if ts is None:
            raise SystemExit("the kernel section gathers from the set of the build section")
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        rng = np.random.default_rng(0)
        store = ts.tiles
        C = store.shape[1]
        index = [torch.from_numpy(rng.integers(0, M, size=N).astype(np.int32)).to(device) for _ in range(a.sets)]
        index64 = [i.long() for i in index]
        starts = [int(rng.integers(0, M - N + 1)) for _ in range(a.sets)]
        dsts = [torch.empty(N, C, S, S, dtype=torch.float32, device=device) for _ in range(a.sets)]
        codes = torch.from_numpy(rng.integers(0, 8, size=N).astype(np.int32)).to(device)
        k = [0]

        def nxt():
            k[0] += 1
            return k[0] % a.sets

        def gather():
            j = nxt()
            _abi.check(lib.rg_tile_gather_transform(store.data_ptr(), M, index[j].data_ptr(), dsts[j].data_ptr(), N, C, S,
                                                    codes.data_ptr(), 0.5, 0.5, st), "tile_gather_transform")
            return dsts[j]

        def two_pass():
            j = nxt()
            x = store.index_select(0, index64[j])
            _abi.check(lib.rg_tile_transform(x.data_ptr(), _abi.RG_U8, dsts[j].data_ptr(), N, C, S, codes.data_ptr(), 0.5, 0.5, st),
                       "tile_transform")
            return dsts[j]

        def contiguous():
            j = nxt()
            _abi.check(lib.rg_tile_transform(store[starts[j]:starts[j] + N].data_ptr(), _abi.RG_U8, dsts[j].data_ptr(), N, C, S,
                                             codes.data_ptr(), 0.5, 0.5, st), "tile_transform")
            return dsts[j]

        variants = {"g_gather_transform": gather, "t_index_select_then_transform": two_pass,
                    "c_tile_transform_contiguous": contiguous, "g#control": gather}
        # same results first: the one launch against the two-pass form on the same index set
        k[0] = 0
        y = gather().clone()
        k[0] = 0
        assert torch.equal(y, two_pass()), "the one launch and the two-pass form differ"
        for fn in variants.values():
            for _ in range(a.sets):
                fn()
        t = interleave(variants, a.rounds, lambda fn: event_us(fn, a.reps, device), "kernel us")
        pixels = N * C * S * S
        kern = {n: stats(v) for n, v in t.items()}
        for n, bytes_pp in (("g_gather_transform", 5), ("t_index_select_then_transform", 7), ("c_tile_transform_contiguous", 5)):
            kern[n]["bytes_per_pixel"] = bytes_pp
            kern[n]["tb_per_s"] = round(bytes_pp * pixels / (kern[n]["median"] * 1e-6) / 1e12, 2)
        gm, tm, cm = (kern[n]["median"] for n in ("g_gather_transform", "t_index_select_then_transform", "c_tile_transform_contiguous"))
        floor = round(abs(kern["g#control"]["median"] - gm), 2)
        res["kernel"] = dict(kern, unit="us per call (device events over %d back-to-back calls, %d rounds)" % (a.reps, a.rounds),
                             store_tiles=M, store_mib=round(store.numel() / 2 ** 20, 1), index_sets=a.sets,
                             destinations_mib=round(a.sets * pixels * 4 / 2 ** 20, 1), noise_floor_us=floor,
                             g_over_t=round(gm / tm, 3), g_over_c=round(gm / cm, 3),
                             g_not_slower_than_t=bool(gm <= tm + floor))

    if "train" not in skip:
        import torch.nn as nn
        from torch.optim import Adam
        import rna_gan_amd as P
        from rna_gan_amd.augment import InputTransform
        scratch = tempfile.mkdtemp(prefix="ab_resident_loader_")      # the Trainer wants a checkpoint directory; nothing is written
        ds = H.SyntheticTiles(a.steps * N, S, 8, False, 7, as_u8=True)
        if ts is not None and len(ts) >= a.steps * N:                  # the same tiles: the build section's set begins with them
            small = DeviceTileSet.from_tensors(ts.tiles[:a.steps * N], labels=ts.labels[:a.steps * N], device=device)
        else:
            small = DeviceTileSet.from_dataset(ds, device)
        fixed = next(iter(DeviceTileLoader(small, N, seed=0, rank=0)))

        def loader_for(name):
            if name == "u8_loader":
                return DataLoader(ds, batch_size=N, num_workers=0, pin_memory=True, drop_last=True), \
                    InputTransform(augment="none", seed=0, rank=0)
            if name == "fixed_batch":
                return FixedBatch(fixed, a.steps), None
            tf = InputTransform(augment="d4" if name == "resident_d4" else "none", seed=0, rank=0)
            return DeviceTileLoader(small, N, transform=tf, seed=0, rank=0), None
        runs = {}
        for name in ("u8_loader", "resident_none", "resident_d4", "fixed_batch"):
            torch.manual_seed(0)
            net = {"generator": {"name": P.DCGANGenerator,
                                 "args": {"encoding_dims": 2048, "out_channels": 3, "step_channels": 64, "out_size": S,
                                          "nonlinearity": nn.LeakyReLU(0.2), "last_nonlinearity": nn.Tanh()},
                                 "optimizer": {"name": Adam, "args": {"lr": 0.0001, "betas": (0.5, 0.999)}}},
                   "discriminator": {"name": P.DCGANDiscriminator,
                                     "args": {"in_size": S, "in_channels": 3, "step_channels": 64, "nonlinearity": nn.LeakyReLU(0.2),
                                              "last_nonlinearity": nn.LeakyReLU(0.2)},
                                     "optimizer": {"name": Adam, "args": {"lr": 0.0004, "betas": (0.5, 0.999)}}}}
            losses = [P.WassersteinGeneratorLoss(), P.WassersteinDiscriminatorLoss(), P.WassersteinGradientPenalty()]
            loader, trainer_tf = loader_for(name)
            tr = P.Trainer(net, losses, checkpoints=os.path.join(scratch, name), sample_size=4,
                           epochs=1, recon=None, device=device, input_transform=trainer_tf)
            tr.save_model = lambda epoch: None                        # a pass is an epoch: time the iterations, not a checkpoint
            runs[name] = (tr, loader)

        def one_pass(run):
            tr, loader = run
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            tr(loader)
            torch.cuda.synchronize(device)
            return a.steps / (time.perf_counter() - t0)
        for run in runs.values():
            one_pass(run)                                             # first launches, graph capture
        t = interleave(runs, a.train_rounds, one_pass, "train it/s")
        tr_res = {n: stats(v) for n, v in t.items()}
        u8 = tr_res["u8_loader"]["median"]
        res["train"] = dict(tr_res, unit="Trainer.train iterations per second", steps_per_pass=a.steps,
                            losses="wgan (stock plugins)", resident_tiles=len(small),
                            resident_none_over_u8=round(tr_res["resident_none"]["median"] / u8, 2),
                            resident_d4_over_u8=round(tr_res["resident_d4"]["median"] / u8, 2),
                            resident_d4_over_fixed_batch=round(tr_res["resident_d4"]["median"] / tr_res["fixed_batch"]["median"], 3),
                            resident_above_u8=bool(min(tr_res["resident_none"]["median"], tr_res["resident_d4"]["median"]) > u8),
                            note="u8_loader draws every tile with numpy on the host (0 workers), as the CLI's synthetic loader "
                                 "does; fixed_batch is the Trainer loop with no input work")

    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
