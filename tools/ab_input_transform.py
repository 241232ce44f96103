#!/usr/bin/env python3
"""The device-side input transform (rg_tile_transform, rna_gan_amd.augment.InputTransform) measured on one device.

    python tools/ab_input_transform.py [--batch 64 --size 256] [--json profiles/input_transform.json]

Sections:
  kernel   the uint8 batch [--batch][3][--size][--size] with mixed per-sample codes, device events around --reps back-to-back
           calls, every variant timed once per round, the order reversed every other round, (a) timed twice per round (the
           difference of its two identically configured timings is the noise floor):
             (a) rg_tile_transform (normalise + D4 in one launch: 1 B read, 4 B written per pixel)
             (b) rg_u8_to_norm alone (the same bytes, no symmetry)
             (c) rg_u8_to_norm, then ONE whole-batch torch.rot90(y, 1, (-2, -1)).contiguous() -- the cheapest form the
                 two-pass route can take (one code for the whole batch; per-sample codes would need a launch per code): 13 B
             (a0) rg_tile_transform with codes == NULL (what --device_transform 1 alone runs)
           The calls rotate over --sets source / destination pairs whose total size exceeds the 256 MiB Infinity Cache, so
           no variant is served from it.  Acceptance: (a) <= (c).
  train    Trainer.train iterations per second over the CLI's synthetic loader (histopathology_gan.SyntheticTiles, stock
           wgan plugins, reference-size networks) under --device_transform 0, --device_transform 1 and --device_transform 1
           --augment d4: one trainer per setting, a warm-up pass each, then --rounds interleaved timed passes of --steps
           iterations (host clock around a pass that ends in a device synchronise; checkpoints are not written).
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
        print("[ab_input_transform] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)),
              file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--train_rounds", type=int, default=3)
    ap.add_argument("--workers", type=int, default=0, help="loader workers of the train section (the CLI's synthetic loader: 0)")
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    from rna_gan_amd import _abi
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    N, S = a.batch, a.size
    res = {"what": "device-side input transform on one device; variants interleaved in one process", "batch": N, "size": S,
           "device": torch.cuda.get_device_name(device)}

    if "kernel" not in skip:
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        rng = np.random.default_rng(0)
        srcs = [torch.from_numpy(rng.integers(0, 256, size=(N, 3, S, S), dtype=np.uint8)).to(device) for _ in range(a.sets)]
        dsts = [torch.empty(N, 3, S, S, dtype=torch.float32, device=device) for _ in range(a.sets)]
        codes = torch.from_numpy(rng.integers(0, 8, size=N).astype(np.int32)).to(device)
        k = [0]

        def pair():
            k[0] += 1
            return srcs[k[0] % a.sets], dsts[k[0] % a.sets]

        def fused(c):
            x, y = pair()
            _abi.check(lib.rg_tile_transform(x.data_ptr(), _abi.RG_U8, y.data_ptr(), N, 3, S, c, 0.5, 0.5, st), "tile_transform")
            return y

        def norm():
            x, y = pair()
            _abi.check(lib.rg_u8_to_norm(x.data_ptr(), y.data_ptr(), x.numel(), 0.5, 0.5, st), "u8_to_norm")
            return y

        variants = {"a_tile_transform": lambda: fused(codes.data_ptr()), "b_u8_to_norm": norm,
                    "c_u8_to_norm_rot90": lambda: torch.rot90(norm(), 1, (-2, -1)).contiguous(),
                    "a0_tile_transform_no_codes": lambda: fused(None), "a#control": lambda: fused(codes.data_ptr())}
        # same results first (and the warm-up of every variant): the fused launch against the two-pass route under one code
        one = torch.full((N,), 1, dtype=torch.int32, device=device)
        x, y = pair()
        _abi.check(lib.rg_tile_transform(x.data_ptr(), _abi.RG_U8, y.data_ptr(), N, 3, S, one.data_ptr(), 0.5, 0.5, st), "tile_transform")
        ref = torch.empty_like(y)
        _abi.check(lib.rg_u8_to_norm(x.data_ptr(), ref.data_ptr(), x.numel(), 0.5, 0.5, st), "u8_to_norm")
        assert torch.equal(y, torch.rot90(ref, 1, (-2, -1)).contiguous()), "the fused launch and the two-pass route differ"
        for fn in variants.values():
            for _ in range(a.sets):
                fn()
        t = interleave(variants, a.rounds, lambda fn: event_us(fn, a.reps, device), "kernel us")
        pixels = N * 3 * S * S
        kern = {n: stats(v) for n, v in t.items()}
        for n, bytes_pp in (("a_tile_transform", 5), ("b_u8_to_norm", 5), ("c_u8_to_norm_rot90", 13), ("a0_tile_transform_no_codes", 5)):
            kern[n]["bytes_per_pixel"] = bytes_pp
            kern[n]["tb_per_s"] = round(bytes_pp * pixels / (kern[n]["median"] * 1e-6) / 1e12, 2)
        am, bm, cm = (kern[n]["median"] for n in ("a_tile_transform", "b_u8_to_norm", "c_u8_to_norm_rot90"))
        res["kernel"] = dict(kern, unit="us per call (device events over %d back-to-back calls, %d rounds)" % (a.reps, a.rounds),
                             buffer_sets=a.sets, working_set_mib=round(a.sets * pixels * 5 / 2 ** 20, 1),
                             noise_floor_us=round(abs(kern["a#control"]["median"] - am), 2),
                             a_over_b=round(am / bm, 3), a_over_c=round(am / cm, 3), a_not_slower_than_c=bool(am <= cm))

    if "train" not in skip:
        import torch.nn as nn
        from torch.optim import Adam
        import histopathology_gan as H
        import rna_gan_amd as P
        from rna_gan_amd.augment import InputTransform
        settings = {"device_transform_0": (0, "none"), "device_transform_1": (1, "none"), "device_transform_1_d4": (1, "d4")}
        runs = {}
        scratch = tempfile.mkdtemp(prefix="ab_input_transform_")      # the Trainer wants a checkpoint directory; nothing is written
        for name, (dt, aug) in settings.items():
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
            tf = InputTransform(augment=aug, seed=0, rank=0) if (dt or aug != "none") else None
            tr = P.Trainer(net, losses, checkpoints=os.path.join(scratch, name), sample_size=4,
                           epochs=1, recon=None, device=device, input_transform=tf)
            tr.save_model = lambda epoch: None                        # a pass is an epoch: time the iterations, not a checkpoint
            ds = H.SyntheticTiles(a.steps * N, S, 8, False, 7, as_u8=bool(dt))
            loader = DataLoader(ds, batch_size=N, num_workers=a.workers, pin_memory=True, drop_last=True)
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
        res["train"] = dict({n: stats(v) for n, v in t.items()}, unit="Trainer.train iterations per second", steps_per_pass=a.steps,
                            loader="histopathology_gan.SyntheticTiles, batch %d, %d workers, pin_memory" % (N, a.workers),
                            losses="wgan (stock plugins)", note="the synthetic loader draws every tile with numpy on the host: "
                            "with 0 workers the rates are bounded by that draw, not by the device")

    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
