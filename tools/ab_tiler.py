#!/usr/bin/env python3
"""The tiler (rg_window_resize_u8, rna_gan_amd.tiler) measured on one device.

    python tools/ab_tiler.py [--windows 512] [--json profiles/tiler_kernels.json]

Sections:
  kernel   --windows windows of 512 -> 256 and of 768 -> 256, the windows a shuffled grid that covers a raster of random bytes (403 MB
           and 906 MB at 512 windows: more than the 256 MiB Infinity Cache, so every call reads its input from memory).  Forms:
           "one_launch" (rg_window_resize_u8: the intermediate in LDS), "two_launch" (rg_probe_window_resize_2pass: the byte
           intermediate in memory), and "one_launch#control", a second identically configured timing of the first (their difference
           is the noise floor).  Device events around --reps back-to-back calls, every form once per round, the order reversed every
           other round.  Before timing, the two forms are compared byte for byte on the whole batch and with PIL.Image.resize on
           --host_windows windows.
  probe    the stream-copy rate of `python -m rna_gan_amd.probe` measured in this process, and the time to stream the bytes a call
           must move (every window read once, every output byte written once) at that rate.
  pillow   a single-thread loop of PIL.Image.resize over --host_windows of the same windows (crops made beforehand), host clock,
           scaled to the batch.
  slide    tiler.tile_raster end to end on a synthetic slide (--slide ROWSxCOLUMNS, patch 256 read at 512), raster already on the
           device, host clock, ends with the tiles on the device and the rows on the host: tiles per second, against the same call on
           a CPU tensor (numpy, one host thread), once.
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
        print("[ab_tiler] %s round %d: %s" % (tag, r, "  ".join("%s %.4g" % (n, out[n][-1]) for n in names)), file=sys.stderr, flush=True)
    return out


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def kernel_section(device, N, read, size, reps, rounds, host_windows, copy_gbps):
    from PIL import Image
    from rna_gan_amd import _abi
    from rna_gan_amd import tiler as TL
    lib = _abi.load()
    gy = 1
    while gy * gy * 2 < N:
        gy *= 2
    gx = -(-N // gy)
    RH, RW = gy * read, gx * read
    g = torch.Generator(device=device).manual_seed(read)
    raster = torch.randint(0, 256, (RH, RW, 3), generator=g, device=device, dtype=torch.uint8)
    grid = np.array([(x * read, y * read) for x in range(gx) for y in range(gy)], dtype=np.int32)
    np.random.RandomState(5).shuffle(grid)
    origins = torch.from_numpy(grid[:N].copy()).to(device)
    table = TL._device_table(read, size, device)
    K = table.shape[1] - 2
    out1 = torch.empty((N, size, size, 3), dtype=torch.uint8, device=device)
    out2 = torch.empty_like(out1)
    ws = torch.empty((N * read * size * 3,), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream

    def one():
        _abi.check(lib.rg_window_resize_u8(raster.data_ptr(), RH, RW, origins.data_ptr(), N, read, read, size, size, table.data_ptr(), K,
                                           table.data_ptr(), K, out1.data_ptr(), 0, stream), "rg_window_resize_u8")

    def two():
        _abi.check(lib.rg_probe_window_resize_2pass(raster.data_ptr(), RH, RW, origins.data_ptr(), N, read, read, size, size,
                                                    table.data_ptr(), K, table.data_ptr(), K, out2.data_ptr(), 0, ws.data_ptr(),
                                                    ws.numel(), stream), "rg_probe_window_resize_2pass")

    one()
    two()
    torch.cuda.synchronize(device)
    assert torch.equal(out1, out2), "the one-launch and the two-launch form differ"
    crops = TL.resize_windows(raster, origins[:host_windows], read, read).cpu().numpy()
    got = out1[:host_windows].cpu().numpy()
    for k in range(crops.shape[0]):
        assert np.array_equal(got[k], np.asarray(Image.fromarray(crops[k]).resize((size, size)))), "window %d differs from Pillow" % k
    variants = {"one_launch": one, "two_launch": two, "one_launch#control": one}
    for fn in variants.values():
        fn()
    t = interleave(variants, rounds, lambda fn: event_us(fn, reps, device), "kernel %d->%d N=%d us" % (read, size, N))
    res = {n: stats(v) for n, v in t.items()}
    in_bytes, out_bytes = N * read * read * 3, N * size * size * 3
    res.update(unit="us per call (device events over %d back-to-back calls, %d rounds)" % (reps, rounds), windows=N, read=read, out=size,
               coefficients_per_pixel=K, raster="%d x %d random bytes" % (RH, RW), input_bytes=in_bytes, output_bytes=out_bytes,
               intermediate_bytes_of_two_launch=N * read * size * 3,
               noise_floor_us=round(abs(res["one_launch#control"]["median"] - res["one_launch"]["median"]), 2),
               two_launch_over_one_launch=round(res["two_launch"]["median"] / res["one_launch"]["median"], 3))
    if copy_gbps:
        # the copy rate counts read + written bytes, as here
        stream_us = (in_bytes + out_bytes) / (copy_gbps * 1e9) * 1e6
        res.update(us_to_stream_input_and_output_at_copy_rate=round(stream_us, 2),
                   one_launch_over_streaming=round(res["one_launch"]["median"] / stream_us, 2))
    # Pillow, one thread
    Image.fromarray(crops[0]).resize((size, size))
    t0 = time.perf_counter()
    for k in range(crops.shape[0]):
        np.asarray(Image.fromarray(crops[k]).resize((size, size)))
    dt = time.perf_counter() - t0
    res["pillow"] = {"what": "PIL.Image.resize in a loop, one host thread, %d windows cropped beforehand" % crops.shape[0],
                     "ms_per_window": round(dt / crops.shape[0] * 1e3, 3), "ms_scaled_to_the_batch": round(dt / crops.shape[0] * N * 1e3, 1),
                     "over_one_launch": round(dt / crops.shape[0] * N * 1e6 / res["one_launch"]["median"], 1)}
    return res


def slide_section(device, shape, rounds):
    from rna_gan_amd import tiler as TL
    a = TL.synthetic_slide(shape[0], shape[1], seed=1, blobs=8, smears=2)
    kw = dict(patch_size=256, app_mag=40.0, thumb_factor=32, max_patches=2000, batch=256)
    cpu = torch.from_numpy(a)
    dev = cpu.to(device)

    def clock(x):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        r = TL.tile_raster(x, **kw)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0, r

    clock(dev)
    times, res = [], None
    for _ in range(rounds):
        dt, res = clock(dev)
        times.append(dt * 1e3)
    dt_cpu, res_cpu = clock(cpu)
    assert torch.equal(res.tiles.cpu(), res_cpu.tiles) and np.array_equal(res.qc, res_cpu.qc), "device and CPU tensor differ"
    med = statistics.median(times)
    return {"slide": "%d x %d synthetic, patch 256 read at 512, thumb factor 32" % shape, "candidates": res.candidates,
            "in_mask": res.in_mask, "examined": res.examined, "tiles": len(res), "device_ms": stats(times),
            "device_tiles_per_s": round(len(res) / (med * 1e-3), 1), "device_windows_examined_per_s": round(res.examined / (med * 1e-3), 1),
            "cpu_tensor_ms": round(dt_cpu * 1e3, 1), "cpu_tensor_tiles_per_s": round(len(res) / dt_cpu, 2),
            "device_over_cpu_tensor": round(dt_cpu * 1e3 / med, 1),
            "unit": "host clock around tiler.tile_raster, raster already in place; the CPU tensor path (numpy, one thread) once"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host_windows", type=int, default=16)
    ap.add_argument("--slide", default="6144x7680")
    ap.add_argument("--slide_rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out (probe, slide)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "the tiler on one device; forms interleaved in one process", "device": torch.cuda.get_device_name(device)}
    gbps = None
    if "probe" not in skip:
        from rna_gan_amd.probe import measure_ceilings
        c = measure_ceilings(device, settle_s=0.5, n_timed=8, copy_mb=1024)
        gbps = c["stream_copy_gbps"]
        res["probe"] = {"stream_copy_gbps": gbps, "stream_copy_what": c["stream_copy_what"]}
        torch.cuda.empty_cache()
    for read in (512, 768):
        res["resize_%d_to_256" % read] = kernel_section(device, a.windows, read, 256, a.reps, a.rounds, a.host_windows, gbps)
        torch.cuda.empty_cache()
    if "slide" not in skip:
        res["tile_raster"] = slide_section(device, tuple(int(v) for v in a.slide.lower().split("x")), a.slide_rounds)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
