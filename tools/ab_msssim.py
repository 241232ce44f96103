#!/usr/bin/env python3
"""Timings of the MS-SSIM kernels (rna_gan_amd.msssim, rg_msssim.hip) on one MI355X.

    python tools/ab_msssim.py [--tiles 2048 --pairs 2048 --size 256] [--json profiles/msssim.json]

Sections:
  kernels   rg_msssim_pyramid over --tiles tiles and rg_msssim_pairs over --pairs random pairs of them, S = 5, timed separately with
            device events over back-to-back calls after a warm-up, --repeats times each (median, min and max are kept): next to the
            time to stream the bytes each reads and writes at the copy rate measured in the same process, and -- the pair launch --
            to its fp64 FMA count at the nominal vector rate.
  torch     the same computation restated with torch on the same device in fp64 (avg_pool2d for the pyramid, grouped conv2d for the
            two passes of the window, the ratios and the means elementwise), over --torch_pairs pairs at a time, in the same process;
            its result is compared with the kernels'.  The pair launch is timed on the same --torch_pairs pairs as well.
            THE CONDITION: the hand-written pair launch must be faster than this by more than the spread of the two measurements.
  metric    one PairDiversity evaluation at --tiles samples with the reference-size generator, next to TissueYield and
            KernelDistance in the same run (host clock around synchronised work).
Nothing here is imported by the product or the tests.  Needs the GPU: there is no fallback."""
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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

NOMINAL_FP64_TFLOPS = 78.6


def events(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def repeated(fn, iters, repeats):
    ts = [events(fn, iters) for _ in range(repeats)]
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "calls_per_timing": iters, "timings": repeats}


def wall(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "timings": repeats}


def torch_components(x, y, S, taps):
    """x, y: uint8 (n, 3, H, W) -> (n, S, 2) fp64 on the device: the definition with torch operators"""
    g = torch.as_tensor(taps, dtype=torch.float64, device=x.device)
    kh, kv = g.view(1, 1, 1, 11).repeat(15, 1, 1, 1), g.view(1, 1, 11, 1).repeat(15, 1, 1, 1)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    x, y = x.double(), y.double()
    out = []
    for s in range(S):
        if s:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        m = F.conv2d(F.conv2d(torch.cat([x, y, x * x, y * y, x * y], dim=1), kh, groups=15), kv, groups=15)
        mx, my, exx, eyy, exy = m[:, 0:3], m[:, 3:6], m[:, 6:9], m[:, 9:12], m[:, 12:15]
        cs = (2.0 * (exy - mx * my) + c2) / ((exx - mx * mx) + (eyy - my * my) + c2)
        l = (2.0 * mx * my + c1) / (mx * mx + my * my + c1)
        out.append(torch.stack([cs.mean(dim=(1, 2, 3)), (l * cs).mean(dim=(1, 2, 3))], dim=1))
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--torch_pairs", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    if not torch.cuda.is_available():
        raise SystemExit("ab_msssim.py measures on the GPU: none found")
    import rna_gan_amd as P
    from rna_gan_amd import _abi, msssim as MS
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, Pn, H = a.tiles, a.pairs, a.size
    S = MS.default_scales(H, H)
    res = {"device": torch.cuda.get_device_name(0), "tiles": N, "pairs": Pn, "size": H, "scales": S, "band": MS.BAND, "cols": MS.COLS,
           "note": "seconds; device events over back-to-back calls after a warm-up (kernels, torch), host clock around synchronised "
                   "work (metric); median, min and max over the repeated timings", "nominal_fp64_tflops": NOMINAL_FP64_TFLOPS}

    def checkpoint(section):
        """a section is done: say so, and keep what is measured so far"""
        print("[ab_msssim] %s done" % section, file=sys.stderr, flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(N, 3, H, H), dtype=np.uint8)
    tiles = torch.from_numpy(base).to(dev)                               # planar, the resident set's layout
    flags = 1
    i, j = MS.random_pairs(N, Pn, 0)
    ia, ib = torch.from_numpy(i.astype(np.int32)).to(dev), torch.from_numpy(j.astype(np.int32)).to(dev)
    lib = _abi.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    per_tile, need = MS._plan(H, H, S, Pn)
    g = (ctypes.c_double * 11)(*MS.taps())

    big = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(big)
    copy = repeated(lambda: dst.copy_(big), 20, a.repeats)
    rate = 2 * big.numel() / copy["median_s"]
    res["copy_rate_GBps"] = rate / 1e9
    del big, dst

    pyr = torch.empty(N * per_tile, dtype=torch.uint8, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((Pn, S, 3, 2), dtype=torch.float64, device=dev)

    def run_pyr():
        _abi.check(lib.rg_msssim_pyramid(tiles.data_ptr(), N, H, H, flags, S, pyr.data_ptr(), N * per_tile, st), "pyramid")

    def run_pairs(n=Pn):
        _abi.check(lib.rg_msssim_pairs(tiles.data_ptr(), pyr.data_ptr(), N, tiles.data_ptr(), pyr.data_ptr(), N, ia.data_ptr(),
                                       ib.data_ptr(), n, H, H, flags, S, g, ws.data_ptr(), need, out.data_ptr(), st), "pairs")
    if "kernels" not in skip:
        t = repeated(run_pyr, 10, a.repeats)
        b = N * 3 * H * H + N * per_tile
        res["pyramid_launch"] = dict(t, bytes=b, stream_s=b / rate, over_stream=t["median_s"] / (b / rate))
        run_pyr()
        t = repeated(run_pairs, 5, a.repeats)
        positions = float(MS.positions(H, H, S).sum()) * 3 * Pn
        # per window position: 55 FMAs of the vertical pass, and 55 of the horizontal pass on (BAND + 10) / BAND as many rows
        fma = positions * 55.0 * (1.0 + (MS.BAND + 10.0) / MS.BAND)
        b = 2 * Pn * (3 * H * H + per_tile) + 2 * need + out.numel() * 8
        res["pair_launch"] = dict(t, bytes=b, stream_s=b / rate, over_stream=t["median_s"] / (b / rate), fma=fma,
                            fp64_tflops=2.0 * fma / t["median_s"] / 1e12, workgroups=need // 16,
                            nominal_fma_s=2.0 * fma / (NOMINAL_FP64_TFLOPS * 1e12), us_per_pair=t["median_s"] / Pn * 1e6)
        checkpoint("kernels")

    if "torch" not in skip:
        n = min(a.torch_pairs, Pn)
        run_pyr()
        ours = repeated(lambda: run_pairs(n), 5, a.repeats)
        run_pairs(n)
        torch.cuda.synchronize()
        mine = (out[:n].cpu().numpy().mean(axis=2) / MS.positions(H, H, S)[None, :, None])
        li, lj = torch.from_numpy(i[:n]).to(dev), torch.from_numpy(j[:n]).to(dev)
        keep = {}

        def run_torch():
            keep["c"] = torch_components(tiles[li], tiles[lj], S, MS.taps())
        theirs = repeated(run_torch, 2, a.repeats)
        diff = float(np.abs(keep["c"].cpu().numpy() - mine).max())
        spread = (ours["max_s"] - ours["min_s"]) + (theirs["max_s"] - theirs["min_s"])
        res["torch_fp64"] = {"pairs": n, "pair_launch": ours, "torch": theirs, "torch_over_kernel": theirs["median_s"] / ours["median_s"],
                             "difference_s": theirs["median_s"] - ours["median_s"], "spread_s": spread,
                             "kernel_faster_by_more_than_the_spread": bool(theirs["min_s"] - ours["max_s"] > 0 and
                                                                           theirs["median_s"] - ours["median_s"] > spread),
                             "max_abs_difference_of_components": diff,
                             "includes": "torch: the gather of the pairs' tiles, the conversion to fp64, the pyramid; kernel: the pair "
                                         "launch alone (its pyramid is built once per tile set, see 'pyramid_launch')"}
        checkpoint("torch")
    del pyr, ws, out

    if "metric" not in skip:
        from rna_gan_amd.metrics import KernelDistance, PairDiversity, TissueYield
        torch.manual_seed(0)
        G = P.DCGANGenerator(encoding_dims=2048, out_channels=3, step_channels=64, out_size=H, nonlinearity=nn.LeakyReLU(0.2),
                             last_nonlinearity=nn.Tanh()).to(dev)
        D = P.DCGANDiscriminator(in_size=H, in_channels=3, step_channels=64, nonlinearity=nn.LeakyReLU(0.2),
                                 last_nonlinearity=nn.LeakyReLU(0.2)).to(dev)
        G.train(); D.train()
        real_f = ((tiles.float() / 255.0 - 0.5) / 0.5)
        div = PairDiversity(N, pairs=Pn, real=tiles, batch_size=256, seed=0)
        qc = TissueYield(N, batch_size=256, seed=0)
        kd = KernelDistance(real_f, batch_size=256, seed=0)
        vals = {}

        def run_div():
            vals["pair_diversity"] = div.metric_ops(G, dev)

        def run_qc():
            vals["tissue_yield"] = qc.metric_ops(G, dev)

        def run_kd():
            vals["kernel_distance"] = kd.metric_ops(G, D, dev)

        def run_gen():
            vals["tiles"] = len(div.generated_tiles(G, dev))
        res["metric_ops"] = {"pair_diversity": wall(run_div, 3), "tissue_yield": wall(run_qc, 3), "kernel_distance": wall(run_kd, 3),
                             "generation_and_export_alone": wall(run_gen, 3), "values": vals, "last": div.last,
                             "what": "%d generated %d^2 tiles per evaluation, reference-size networks, the real baseline cached" % (N, H)}

    checkpoint("all")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
