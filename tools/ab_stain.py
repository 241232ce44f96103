#!/usr/bin/env python3
"""Macenko stain normalisation on the device (rg_stain.hip, rna_gan_amd.stain) measured on one device.

    python tools/ab_stain.py [--batch 512 --size 256] [--json profiles/stain_kernels.json]

Sections:
  kernel   uint8 tiles [batch][--size][--size][3], synthetic Beer-Lambert H&E (two stains, gamma concentrations, a quarter
           background, sensor noise).  Each of the four entry points alone, with the host operands of a fit of the first set: device
           events around --reps back-to-back calls, every variant timed once per round, the order reversed every other round, the
           moments kernel timed twice per round (the difference is the noise floor).  The calls rotate over tile sets whose total
           size exceeds the 256 MiB Infinity Cache.  Bytes moved per pixel: 3 read by each statistics kernel, 3 read + 3 written by
           rg_stain_apply.  Next to each time: the time to move those bytes at the stream-copy rate.
  probe    the stream-copy rate of `python -m rna_gan_amd.probe` measured in this process.
  end      stain.fit + stain.normalize end to end (host clock, the three downloads and the host arithmetic included) on the device
           tiles, and the numpy path on --host_tiles of the same tiles on a CPU tensor, scaled to the batch.
Nothing here is imported by the product or the tests."""
import argparse
import ctypes
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


def stats(v, digits=2):
    return {"all": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits)}


def make_tiles(N, S, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    he = torch.tensor([[0.65, 0.07], [0.70, 0.99], [0.29, 0.11]], device=device)
    he = he / he.norm(dim=0, keepdim=True)
    u = torch.rand((N, S, S, 4), generator=g, device=device).clamp_min_(1e-6)
    conc = torch.stack([-(u[..., 0] * u[..., 1]).log() * 0.45, -(u[..., 2] * u[..., 3]).log() * 0.3], dim=-1)      # Gamma(2, .)
    conc = conc * (torch.rand((N, S, S, 1), generator=g, device=device) >= 0.25)
    img = 240.0 * torch.exp(-(conc @ he.T)) + 1.5 * torch.randn((N, S, S, 3), generator=g, device=device)
    return img.round_().clamp_(0, 255).to(torch.uint8).contiguous()


def kernel_section(device, N, S, reps, rounds):
    from rna_gan_amd import _abi, stain
    lib = _abi.load()
    pixels = N * S * S
    sets = max(2, -(-(320 << 20) // (3 * pixels)) + 1)
    data = [make_tiles(N, S, device, 31 * i) for i in range(sets)]
    small = data[0][:4]
    fs = stain.fit(small)
    assert fs == stain.fit(small.cpu()), "device fit and numpy fit differ"
    assert torch.equal(stain.normalize(small, fs).cpu(), stain.normalize(small.cpu(), fs)), "device and numpy bytes differ"
    f = stain.fit(data[0])
    D = stain._Device.get(device)                                              # its accumulators hold the integers of that fit
    e1, e2 = stain.basis_from_moments(D.acc[:10].cpu().numpy())
    basis6 = stain._ii(stain.quantize_basis(e1, e2))
    pinv6, scale2, href6 = stain.apply_operands(f, stain.REFERENCE_TARGET)
    p6, s2, h6 = stain._ll(pinv6), stain._ll(scale2), stain._ii(href6)
    out = torch.empty_like(data[0])
    st = torch.cuda.current_stream(device).cuda_stream
    k = [0]

    def src():
        k[0] += 1
        return data[k[0] % sets].data_ptr()

    def moments():
        _abi.check(lib.rg_stain_moments(src(), N, S, S, 0, D.od.data_ptr(), stain.beta_q(), D.acc.data_ptr(), 0, st), "moments")

    def angle():
        _abi.check(lib.rg_stain_angle_hist(src(), N, S, S, 0, D.od.data_ptr(), stain.beta_q(), basis6, D.dirs.data_ptr(),
                                           stain.K, D.acc[10:].data_ptr(), 0, st), "angle")

    def conc():
        _abi.check(lib.rg_stain_conc_hist(src(), N, S, S, 0, D.od.data_ptr(), p6, stain.QP, stain.CSH, stain.CB,
                                          D.acc[10 + stain.K + 1:].data_ptr(), 0, st), "conc")

    def apply():
        _abi.check(lib.rg_stain_apply(src(), out.data_ptr(), N, S, S, 0, D.od.data_ptr(), p6, stain.QP, s2,
                                      stain.QS, h6, stain.QH + stain.QOD - stain.QO, D.out.data_ptr(), D.L, D.off, st), "apply")

    def copy():
        out.copy_(data[(k[0] + 1) % sets])
        k[0] += 1

    variants = {"moments": moments, "angle_hist": angle, "conc_hist": conc, "apply": apply, "torch_copy": copy, "moments#control": moments}
    for fn in variants.values():
        for _ in range(sets):
            fn()
    names = list(variants)
    t = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            t[n].append(event_us(variants[n], reps, device))
        print("[ab_stain] round %d: %s" % (r, "  ".join("%s %.4g" % (n, t[n][-1]) for n in names)), file=sys.stderr, flush=True)
    res = {n: stats(v) for n, v in t.items()}
    moved = {"moments": 3, "angle_hist": 3, "conc_hist": 3, "apply": 6, "torch_copy": 6}
    for n, b in moved.items():
        res[n]["bytes_per_pixel"] = b
        res[n]["tb_per_s"] = round(b * pixels / (res[n]["median"] * 1e-6) / 1e12, 3)
    return dict(res, unit="us per call (device events over %d back-to-back calls, %d rounds)" % (reps, rounds), batch=N, size=S,
                pixels=pixels, buffer_sets=sets, noise_floor_us=round(abs(res["moments#control"]["median"] - res["moments"]["median"]), 2),
                stained_share=round(f.n_stained / f.n_pixels, 4)), data[0], f


def end_section(device, tiles, host_tiles, rounds):
    from rna_gan_amd import stain
    N = tiles.shape[0]

    def dev():
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        f = stain.fit(tiles)
        t1 = time.perf_counter()
        stain.normalize(tiles, f)
        torch.cuda.synchronize(device)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    dev()
    d = [dev() for _ in range(rounds)]
    cpu = tiles[:host_tiles].cpu()
    t0 = time.perf_counter()
    f = stain.fit(cpu)
    t1 = time.perf_counter()
    stain.normalize(cpu, f)
    t2 = time.perf_counter()
    fit_ms, norm_ms = statistics.median(x[0] for x in d), statistics.median(x[1] for x in d)
    return {"device_fit_ms": round(fit_ms, 3), "device_normalize_ms": round(norm_ms, 3), "device_total_ms": round(fit_ms + norm_ms, 3),
            "numpy_what": "the numpy path of rna_gan_amd.stain on %d of the tiles on a CPU tensor (one host thread), scaled to %d" % (host_tiles, N),
            "numpy_fit_ms_scaled": round((t1 - t0) * 1e3 * N / host_tiles, 1), "numpy_normalize_ms_scaled": round((t2 - t1) * 1e3 * N / host_tiles, 1),
            "numpy_over_device": round(((t2 - t0) * 1e3 * N / host_tiles) / (fit_ms + norm_ms), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host_tiles", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "Macenko stain normalisation on one device; variants interleaved in one process", "device": torch.cuda.get_device_name(device)}
    res["kernel"], tiles, _ = kernel_section(device, a.batch, a.size, a.reps, a.rounds)
    res["end_to_end"] = end_section(device, tiles, a.host_tiles, 5)
    del tiles
    torch.cuda.empty_cache()
    from rna_gan_amd.probe import measure_ceilings
    c = measure_ceilings(device, settle_s=0.5, n_timed=8, copy_mb=1024)
    gbps = c["stream_copy_gbps"]
    res["probe"] = {"stream_copy_gbps": gbps, "stream_copy_what": c["stream_copy_what"]}
    for n in ("moments", "angle_hist", "conc_hist", "apply"):
        kk = res["kernel"][n]
        kk["us_at_copy_rate"] = round(kk["bytes_per_pixel"] * res["kernel"]["pixels"] / (gbps * 1e9) * 1e6, 2)
        kk["over_copy_rate"] = round(kk["median"] / kk["us_at_copy_rate"], 2)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
