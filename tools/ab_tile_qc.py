#!/usr/bin/env python3
"""Tile quality control on the device (rg_tile_qc, rna_gan_amd.tissue) measured on one device.

    python tools/ab_tile_qc.py [--batch 512 --size 256] [--samples 2048] [--json profiles/tile_qc.json]

Sections:
  kernel   uint8 tiles [batch][--size][--size][3] of three contents -- "tissue" (a bright, nearly grey background with saturated
           blobs: what an H&E tile looks like to the histograms), "noise" (uniform bytes: every bin of every histogram occupied) and
           "constant" (one colour: every pixel of a tile lands in ONE bin of each histogram, the worst case for the LDS atomics).
           Device events around --reps back-to-back WHOLE calls (all five launches), every variant timed once per round, the order
           reversed every other round, the tissue variant timed twice per round (the difference of its two identically configured
           timings is the noise floor).  The calls rotate over tile sets whose total size exceeds the 256 MiB Infinity Cache.
           The results of every variant are first compared with the CPU path on a few tiles.
  host     (a) the numpy restatement the CPU path runs (rna_gan_amd.tissue._tile_stats_numpy) on --host_tiles of the same tissue
           tiles, host clock; reported per tile and scaled to the batch.
  probe    (b) the stream-copy rate of `python -m rna_gan_amd.probe` measured in this process, and the time to stream the batch's
           bytes once at that rate, times the number of reads of the launch plan (2).
  metric   (c) what TissueYield adds per evaluation at --samples generated tiles of the reference-size generator (bf16), next to a
           KernelDistance evaluation over the same number of tiles in the same process: host clock around metric_ops (each ends
           with its values on the host), interleaved rounds; and the part of TissueYield that is not the generator (export +
           rg_tile_qc + the download of 48 bytes per tile) timed on tiles generated beforehand.
Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

READS = 2          # how often the launch plan reads the tile bytes from memory (tq_hist, tq_mask; plus the dilation halo)


def event_us(fn, reps, device):
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
        print("[ab_tile_qc] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)),
              file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def make_tiles(kind, N, S, device, seed):
    """uint8 [N][S][S][3] on the device, from a seeded device generator"""
    g = torch.Generator(device=device).manual_seed(seed)
    if kind == "noise":
        return torch.randint(0, 256, (N, S, S, 3), generator=g, device=device, dtype=torch.uint8)
    if kind == "constant":
        col = torch.randint(60, 256, (N, 1, 1, 3), generator=g, device=device, dtype=torch.uint8)
        return col.expand(N, S, S, 3).contiguous()
    grey = torch.randint(215, 256, (N, S, S, 1), generator=g, device=device, dtype=torch.int16)
    x = grey + torch.randint(-6, 7, (N, S, S, 3), generator=g, device=device, dtype=torch.int16)
    lo = torch.tensor([120, 40, 110], device=device, dtype=torch.int16)
    span = torch.tensor([100, 100, 90], device=device, dtype=torch.float32)
    blob = (lo + (torch.rand((N, S, S, 3), generator=g, device=device) * span).to(torch.int16))
    # smooth blobs: a low-resolution random field, upsampled, thresholded per tile
    field = torch.rand((N, 1, max(S // 32, 1), max(S // 32, 1)), generator=g, device=device)
    field = torch.nn.functional.interpolate(field, size=(S, S), mode="bilinear", align_corners=False)[:, 0, :, :, None]
    x = torch.where(field > 0.55, blob, x)
    return x.clamp_(0, 255).to(torch.uint8).contiguous()


def kernel_section(device, N, S, reps, rounds):
    from rna_gan_amd import tissue as TQ
    tile_bytes = N * S * S * 3
    sets = max(2, -(-(320 << 20) // tile_bytes) + 1)
    kinds = ("tissue", "noise", "constant")
    data = {k: [make_tiles(k, N, S, device, 17 * i + j) for i in range(sets)] for j, k in enumerate(kinds)}
    out_rows = torch.empty((N, 12), dtype=torch.int32, device=device)
    k = [0]

    def call(kind):
        k[0] += 1
        TQ.tile_stats_device(data[kind][k[0] % sets], out=out_rows)

    # same results first
    summary = {}
    for kind in kinds:
        t = data[kind][0][:4]
        dev = TQ.tile_stats(t)
        cpu = TQ.tile_stats(t.cpu())
        assert np.array_equal(dev.stats, cpu.stats), "rg_tile_qc and the CPU path differ on %s tiles" % kind
        full = TQ.tile_stats(data[kind][0])
        summary[kind] = {"accepted": round(float(TQ.accept(full).mean()), 4), "tissue_fraction": round(float(TQ.tissue_fraction(full).mean()), 4),
                         "low_contrast": round(float(TQ.low_contrast(full).mean()), 4)}
    variants = {"tissue": lambda: call("tissue"), "noise": lambda: call("noise"), "constant": lambda: call("constant"),
                "tissue#control": lambda: call("tissue")}
    for fn in variants.values():
        for _ in range(sets):
            fn()
    t = interleave(variants, rounds, lambda fn: event_us(fn, reps, device), "kernel N=%d us" % N)
    kern = {n: stats(v) for n, v in t.items()}
    for n in kinds:
        kern[n]["tb_per_s_of_%d_reads" % READS] = round(READS * tile_bytes / (kern[n]["median"] * 1e-6) / 1e12, 3)
        kern[n]["content"] = summary[n]
    return dict(kern, unit="us per whole rg_tile_qc call (device events over %d back-to-back calls, %d rounds)" % (reps, rounds),
                batch=N, size=S, tile_bytes=tile_bytes, buffer_sets=sets, reads_of_the_tile_bytes=READS,
                noise_floor_us=round(abs(kern["tissue#control"]["median"] - kern["tissue"]["median"]), 2)), data["tissue"][0]


def host_section(tiles, n_host, N):
    from rna_gan_amd import tissue as TQ
    a = tiles[:n_host].cpu().numpy()
    ranks, _ = TQ.percentile_ranks(a.shape[1] * a.shape[2])
    TQ._tile_stats_numpy(a[:2], 50, 3, ranks, False)
    t0 = time.perf_counter()
    TQ._tile_stats_numpy(a, 50, 3, ranks, False)
    dt = time.perf_counter() - t0
    return {"what": "rna_gan_amd.tissue._tile_stats_numpy (numpy; one host thread) on %d of the tissue tiles" % a.shape[0],
            "ms_per_tile": round(dt / a.shape[0] * 1e3, 3), "ms_scaled_to_the_batch": round(dt / a.shape[0] * N * 1e3, 1)}


def probe_section(device, tile_bytes):
    from rna_gan_amd.probe import measure_ceilings
    c = measure_ceilings(device, settle_s=0.5, n_timed=8, copy_mb=1024)
    gbps = c["stream_copy_gbps"]
    once_us = tile_bytes / (gbps * 1e9) * 1e6
    return {"stream_copy_gbps": gbps, "stream_copy_what": c["stream_copy_what"], "us_to_stream_the_batch_once": round(once_us, 2),
            "reads": READS, "us_for_the_reads_of_the_plan": round(READS * once_us, 2)}


def metric_section(device, samples, S, rounds):
    import torch.nn as nn
    import rna_gan_amd as P
    from rna_gan_amd import synth
    from rna_gan_amd import tissue as TQ
    from rna_gan_amd.metrics import KernelDistance, TissueYield
    G = P.DCGANGenerator(2048, S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
    D = P.DCGANDiscriminator(S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2))
    synth.seeded_fill_(G, 3)
    synth.seeded_fill_(D, 4)
    G, D = G.set_precision("bf16").to(device).train(), D.set_precision("bf16").to(device).train()
    real = make_tiles("tissue", samples, S, device, 99).permute(0, 3, 1, 2).contiguous()          # uint8 NCHW
    kid = KernelDistance(real, batch_size=256, seed=1)
    qc = TissueYield(samples, batch_size=256, seed=1)
    tiles = torch.cat(qc.generated_tiles(G, device))

    def qc_only():
        rows = [TQ.tile_stats_device(c)[0] for c in torch.split(tiles, 256)]
        return torch.cat(rows).cpu()

    def clock(fn):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        return (time.perf_counter() - t0) * 1e3

    variants = {"kernel_distance": lambda: kid.metric_ops(G, D, device), "tissue_yield": lambda: qc.metric_ops(G, device),
                "tile_qc_and_download_only": qc_only, "tissue_yield#control": lambda: qc.metric_ops(G, device)}
    for fn in variants.values():
        fn()
    t = interleave(variants, rounds, clock, "metric ms")
    out = {n: stats(v) for n, v in t.items()}
    return dict(out, unit="ms per evaluation (host clock, ends with the values on the host; %d rounds)" % rounds, samples=samples,
                networks="DCGANGenerator(2048, %d, 3, 64) / DCGANDiscriminator(%d, 3, 64), bf16, seeded weights" % (S, S),
                tissue_yield_last=qc.last,
                noise_floor_ms=round(abs(out["tissue_yield#control"]["median"] - out["tissue_yield"]["median"]), 2),
                tissue_yield_over_kernel_distance=round(out["tissue_yield"]["median"] / out["kernel_distance"]["median"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host_tiles", type=int, default=32)
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--metric_rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out (host, probe, metric)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "tile quality control on one device; variants interleaved in one process",
           "device": torch.cuda.get_device_name(device)}
    res["kernel"], tissue = kernel_section(device, a.batch, a.size, a.reps, a.rounds)
    if "host" not in skip:
        res["host"] = host_section(tissue, a.host_tiles, a.batch)
    del tissue
    torch.cuda.empty_cache()
    if "probe" not in skip:
        res["probe"] = probe_section(device, res["kernel"]["tile_bytes"])
        res["call_over_the_reads_at_copy_rate"] = round(res["kernel"]["tissue"]["median"] / res["probe"]["us_for_the_reads_of_the_plan"], 2)
        torch.cuda.empty_cache()
    if "metric" not in skip:
        res["metric"] = metric_section(device, a.samples, a.size, a.metric_rounds)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
