#!/usr/bin/env python3
"""The device-side tile export (rg_tile_export_u8, rna_gan_amd.export) measured on one device.

    python tools/ab_tile_export.py [--batches 64,512 --size 256] [--samples 4096 --chunk 512] [--json profiles/tile_export.json]

Sections:
  kernel   per batch size, fp32 images [batch][3][--size][--size]; device events around --reps back-to-back calls, every variant
           timed once per round, the order reversed every other round, (b) timed twice per round (the difference of its two
           identically configured timings is the noise floor):
             (a)  rg_tile_export_u8, interleaved RGB, rounding rule (12 B read + 3 B written per pixel)
             (a1) rg_tile_export_u8, planar
             (b)  rg_export_images_nhwc on the same input (12 B read + 12 B written per pixel)
             (c)  the float4 stream copy of the same fp32 bytes (rg_probe_copy: 12 B read + 12 B written per pixel)
           The calls rotate over source / destination sets whose total size exceeds the 256 MiB Infinity Cache, so no variant is
           served from it.  Acceptance: (a) <= (b) + the noise floor.  (a) is also reported as TB/s of its 15 bytes next to (c).
  host     --samples tiles from the reference-size generator (bf16, seeded weights), delivered to host memory in chunks of --chunk:
             route1  what generate_images does per chunk: synthesize -> export_images_nhwc -> .cpu()  (12 B per pixel on the link)
             route2  export.synthesize_u8                                                      (3 B per pixel on the link)
             device  synthesize alone, the output left on the device
           host clock around a pass that ends with every byte on the host (route1 / route2) or in a device synchronise (device);
           interleaved rounds with a control copy of route1.  Acceptance: route2 delivers at least as many imgs/s as route1.
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
        print("[ab_tile_export] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)),
              file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def kernel_section(lib, _abi, device, N, S, reps, rounds):
    st = torch.cuda.current_stream(device).cuda_stream
    pixels = N * S * S
    src_bytes = pixels * 12
    sets = max(2, -(-(320 << 20) // (src_bytes * 2)) + 1)          # sources + fp32 destinations past 256 MiB, with a margin
    gen = torch.Generator(device="cpu").manual_seed(N)
    base = torch.empty(N, 3, S, S, dtype=torch.float32).uniform_(-1.1, 1.1, generator=gen)
    srcs = [base.roll(i, 0).to(device) for i in range(sets)]
    f32 = [torch.empty(N, S, S, 3, dtype=torch.float32, device=device) for _ in range(sets)]
    u8 = [torch.empty(N, S, S, 3, dtype=torch.uint8, device=device) for _ in range(sets)]
    k = [0]

    def nxt():
        k[0] += 1
        return k[0] % sets

    def export(flags):
        i = nxt()
        _abi.check(lib.rg_tile_export_u8(srcs[i].data_ptr(), u8[i].data_ptr(), N, 3, S, S, -1.0, 2.0, flags, st), "tile_export_u8")
        return u8[i]

    def nhwc():
        i = nxt()
        _abi.check(lib.rg_export_images_nhwc(srcs[i].data_ptr(), f32[i].data_ptr(), N, 3, S, S, st), "export_images_nhwc")
        return f32[i]

    def copy():
        i = nxt()
        _abi.check(lib.rg_probe_copy(srcs[i].data_ptr(), f32[i].data_ptr(), src_bytes, 0, 0, st), "probe_copy")

    # same results first: the new launch against the existing kernel's value, quantised by torch
    got = export(0)
    j = k[0] % sets
    ref = torch.empty_like(f32[j])
    _abi.check(lib.rg_export_images_nhwc(srcs[j].data_ptr(), ref.data_ptr(), N, 3, S, S, st), "export_images_nhwc")
    want = ref.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    assert torch.equal(got, want), "rg_tile_export_u8 and the quantised rg_export_images_nhwc differ"
    del ref, want
    variants = {"a_export_u8_rgb": lambda: export(0), "a1_export_u8_planar": lambda: export(1), "b_export_images_nhwc": nhwc,
                "c_stream_copy": copy, "b#control": nhwc}
    for fn in variants.values():
        for _ in range(sets):
            fn()
    t = interleave(variants, rounds, lambda fn: event_us(fn, reps, device), "kernel N=%d us" % N)
    kern = {n: stats(v) for n, v in t.items()}
    for n, bpp in (("a_export_u8_rgb", 15), ("a1_export_u8_planar", 15), ("b_export_images_nhwc", 24), ("c_stream_copy", 24)):
        kern[n]["bytes_per_pixel"] = bpp
        kern[n]["tb_per_s"] = round(bpp * pixels / (kern[n]["median"] * 1e-6) / 1e12, 2)
    am, bm = kern["a_export_u8_rgb"]["median"], kern["b_export_images_nhwc"]["median"]
    floor = round(abs(kern["b#control"]["median"] - bm), 2)
    return dict(kern, unit="us per call (device events over %d back-to-back calls, %d rounds)" % (reps, rounds), batch=N,
                buffer_sets=sets, working_set_mib=round(sets * src_bytes * 2 / 2 ** 20, 1), noise_floor_us=floor,
                a_over_b=round(am / bm, 3), a_not_slower_than_b=bool(am <= bm + floor),
                a_tb_per_s_over_stream_copy=round(kern["a_export_u8_rgb"]["tb_per_s"] / kern["c_stream_copy"]["tb_per_s"], 3))


def host_section(device, samples, chunk, S, rounds):
    import torch.nn as nn
    import rna_gan_amd as P
    from rna_gan_amd import export as EX
    from rna_gan_amd import synth
    from rna_gan_amd.gan_utils import synthesize
    G = P.DCGANGenerator(2048, S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh())
    synth.seeded_fill_(G, 3)
    G = G.set_precision("bf16").to(device).eval()
    ops, _ = G.runtime()
    noise = torch.randn(samples, 2048, generator=torch.Generator().manual_seed(7)).to(device)

    def route1():
        n = 0
        for c in torch.split(noise, chunk):
            a = ops.export_images_nhwc(synthesize(G, c, chunk=chunk)).cpu().numpy()
            n += a.shape[0]
        return n

    def route2():
        n = 0
        for _start, a in EX.synthesize_u8(G, noise, chunk=chunk):
            n += a.shape[0]
        return n

    def on_device():
        for c in torch.split(noise, chunk):
            synthesize(G, c, chunk=chunk)
        return samples

    def rate(fn):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize(device)
        return n / (time.perf_counter() - t0)

    # same tiles first: route 2's bytes are route 1's values under the rounding rule
    a = ops.export_images_nhwc(synthesize(G, noise[:chunk], chunk=chunk)).cpu()
    want = a.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    got = next(iter(EX.synthesize_u8(G, noise[:chunk], chunk=chunk)))[1]
    assert np.array_equal(got, want), "route 2 does not deliver route 1's tiles"
    variants = {"route1_f32_nhwc_cpu": route1, "route2_synthesize_u8": route2, "device_synthesize_only": on_device,
                "route1#control": route1}
    for fn in variants.values():
        fn()
    t = interleave(variants, rounds, rate, "host imgs/s")
    out = {n: stats(v, 1) for n, v in t.items()}
    r1, r2 = out["route1_f32_nhwc_cpu"]["median"], out["route2_synthesize_u8"]["median"]
    px = S * S
    out["route1_f32_nhwc_cpu"]["link_gb_per_s"] = round(r1 * px * 12 / 1e9, 2)
    out["route2_synthesize_u8"]["link_gb_per_s"] = round(r2 * px * 3 / 1e9, 2)
    return dict(out, unit="images per second delivered to host memory (host clock, %d rounds)" % rounds, samples=samples, chunk=chunk,
                generator="DCGANGenerator(2048, %d, 3, 64), bf16, eval-mode BatchNorm folded" % S,
                noise_floor_imgs_per_s=round(abs(out["route1#control"]["median"] - r1), 1),
                route2_over_route1=round(r2 / r1, 3), route2_not_slower_than_route1=bool(r2 >= r1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--host_rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    from rna_gan_amd import _abi
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "device-side tile export on one device; variants interleaved in one process", "size": a.size,
           "device": torch.cuda.get_device_name(device)}
    if "kernel" not in skip:
        lib = _abi.load()
        res["kernel"] = [kernel_section(lib, _abi, device, int(n), a.size, a.reps, a.rounds) for n in a.batches.split(",")]
        torch.cuda.empty_cache()
    if "host" not in skip:
        res["host"] = host_section(device, a.samples, a.chunk, a.size, a.host_rounds)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
