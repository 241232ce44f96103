#!/usr/bin/env python3
"""The precision / recall / density / coverage evaluation (rna_gan_amd.prdc, metrics.PrecisionRecall) measured on one device,
with the interleaving scheme of tools/ab_fd_eval.py: per round every variant is timed once, the order is reversed every other
round, and the baseline is timed twice per round -- the difference of its two identically configured timings is the noise floor.

    python tools/ab_prdc_eval.py --rows 2048 --features 2048 [--images 2048 --size 256] [--json profiles/prdc_device_eval.json]

Sections:
  kernels     rg_knn_radii2 (k = 5) and rg_radius_hits (with radii, and the minimum alone) at (na, nb, F) = (--rows, --rows,
              --features): time of the call (tile kernel + merge kernel) and fp64 TFLOP/s at 3 F flops per computed pair (a
              subtraction and a fused multiply-add; rg_knn_radii2 computes T (T + 1) / 2 of the T^2 tiles), next to the nominal
              78.6 TFLOP/s and to rg_polykernel_tile_sums' two-operand form in the same process (2 F flops per pair: one
              instruction per element pair where the distance kernels issue two);
  prdc        prdc.prdc on --rows + --rows device features against the plain-torch formulation ON THE SAME DEVICE: torch.cdist
              in fp64 (the three m x n matrices in memory), topk and comparisons;
  metric      PrecisionRecall.metric_ops next to KernelDistance.metric_ops with the reference-size networks and --images real
              tiles on the device: the per-epoch cost of --pr_samples next to --kid_samples.
The feature's claim is the exact, order-free contract and the absence of an n x n fp64 matrix, not a speed ratio: the JSON says
which formulation was faster.  Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ab_fd_eval import interleave, summary  # noqa: E402

NOMINAL_FP64_TFLOPS = 78.6


def torch_prdc(x, y, k):
    """the four values from fp64 distance matrices held in memory (torch.cdist, topk, comparisons) -- the usual formulation"""
    xd, yd = x.double(), y.double()
    dxx, dyy, dxy = torch.cdist(xd, xd), torch.cdist(yd, yd), torch.cdist(xd, yd)
    rx = dxx.topk(k + 1, dim=1, largest=False).values[:, k]          # the row itself is the smallest entry
    ry = dyy.topk(k + 1, dim=1, largest=False).values[:, k]
    in_real = dxy <= rx[:, None]                                       # [i][j]: y_j inside the ball of x_i
    in_fake = dxy <= ry[None, :]
    m, n = x.shape[0], y.shape[0]
    four = torch.stack([in_real.any(dim=0).sum().double() / n, in_fake.any(dim=1).sum().double() / m,
                        in_real.sum().double() / (float(k) * n), (dxy.min(dim=1).values <= rx).sum().double() / m]).cpu().tolist()
    return dict(zip(("precision", "recall", "density", "coverage"), four))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    import rna_gan_amd as P
    from rna_gan_amd import _abi, kid as K, prdc as PR, probe
    from rna_gan_amd.metrics import KernelDistance, PrecisionRecall
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    n, Fdim, k = a.rows, a.features, a.k
    res = {"what": "precision / recall / density / coverage evaluation on one device; variants interleaved in one process",
           "rows_per_set": n, "features": Fdim, "k": k, "rounds": a.rounds, "nominal_fp64_tflops": NOMINAL_FP64_TFLOPS}
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, Fdim, generator=gen).to(device)
    y = (torch.randn(n, Fdim, generator=gen) * 1.1 + 0.05).to(device)

    if "kernels" not in skip:
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        T = K._tiles(n)
        need = max(lib.rg_pairdist_ws_bytes(n, n, k), lib.rg_pairdist_ws_bytes(n, n, 0))
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        r2 = torch.empty(n, dtype=torch.float64, device=device)
        count = torch.empty(n, dtype=torch.int32, device=device)
        mind2 = torch.empty(n, dtype=torch.float64, device=device)
        sums = torch.zeros(T, T, dtype=torch.float64, device=device)
        _abi.check(lib.rg_knn_radii2(y.data_ptr(), Fdim, n, Fdim, k, ws.data_ptr(), need, r2.data_ptr(), st), "knn")
        calls = (("rg_knn_radii2", "k=%d, upper triangle" % k, T * (T + 1) // 2 * 4096, 3.0,
                  lambda: lib.rg_knn_radii2(x.data_ptr(), Fdim, n, Fdim, k, ws.data_ptr(), need, mind2.data_ptr(), st)),
                 ("rg_radius_hits", "counts and minima", T * T * 4096, 3.0,
                  lambda: lib.rg_radius_hits(x.data_ptr(), Fdim, n, y.data_ptr(), Fdim, n, Fdim, r2.data_ptr(), ws.data_ptr(), need,
                                             count.data_ptr(), mind2.data_ptr(), st)),
                 ("rg_radius_hits", "minima only", T * T * 4096, 3.0,
                  lambda: lib.rg_radius_hits(x.data_ptr(), Fdim, n, y.data_ptr(), Fdim, n, Fdim, None, ws.data_ptr(), need, None,
                                             mind2.data_ptr(), st)),
                 ("rg_polykernel_tile_sums", "two-operand", T * T * 4096, 2.0,
                  lambda: lib.rg_polykernel_tile_sums(x.data_ptr(), Fdim, n, y.data_ptr(), Fdim, n, Fdim, 1.0 / Fdim, 1.0, 3,
                                                      sums.data_ptr(), None, st)))
        rows = []
        for name, form, pairs, flops, call in calls:
            ms = probe._timed(lambda: _abi.check(call(), name), 0.3, 16, device)
            rows.append({"kernel": name, "form": form, "na": n, "nb": n, "F": Fdim, "us": round(ms * 1e3, 1),
                         "flops_per_pair_and_feature": flops, "fp64_tflops": round(flops * pairs * Fdim / (ms * 1e-3) / 1e12, 2)})
        res["kernels"] = rows
        res["hits_over_polykernel_time"] = round(rows[1]["us"] / rows[3]["us"], 2)
        res["expectation"] = ("two fp64 instructions per element pair against the Gram sums' one: about twice the two-operand "
                              "rg_polykernel_tile_sums time (566 us at 2048 x 2048 x 2048 in profiles/kid_device_eval.json)")

    if "prdc" not in skip:
        keep = {}

        def plain():
            keep["torch"] = torch_prdc(x, y, k)

        def dev():
            keep["device"] = PR.prdc(x, y, k=k)
        plain(); dev()
        torch.cuda.reset_peak_memory_stats(device)
        base = torch.cuda.memory_allocated(device)
        dev()
        peak_dev = torch.cuda.max_memory_allocated(device) - base
        torch.cuda.reset_peak_memory_stats(device)
        plain()
        peak_torch = torch.cuda.max_memory_allocated(device) - base
        t = interleave({"torch": plain, "device": dev, "torch#control": plain}, a.rounds, device, "prdc")
        s = summary(t, host="torch", dev="device", control="torch#control")
        s["torch_over_device"] = s.pop("host_over_device")
        res["prdc"] = dict(s, what="prdc.prdc (named device) against torch.cdist in fp64 + topk + comparisons on the same device (named "
                                   "torch)", values=keep, peak_extra_bytes={"device": int(peak_dev), "torch": int(peak_torch)},
                           faster="device" if s["device_not_slower"] else "torch")

    if "metric" not in skip:
        N, S = a.images, a.size
        rng = np.random.default_rng(0)
        u8 = rng.integers(0, 256, size=(N, S, S, 3), dtype=np.uint8)
        real = ((torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).to(device)
        G = P.DCGANGenerator(encoding_dims=2048, out_channels=3, step_channels=64, out_size=S, nonlinearity=nn.LeakyReLU(0.2),
                             last_nonlinearity=nn.Tanh()).to(device)
        D = P.DCGANDiscriminator(in_size=S, in_channels=3, step_channels=64, nonlinearity=nn.LeakyReLU(0.2),
                                 last_nonlinearity=nn.LeakyReLU(0.2)).to(device)
        G.train(); D.train()
        kd, pr = KernelDistance(real, batch_size=256, seed=0), PrecisionRecall(real, batch_size=256, seed=0, nearest_k=k)
        vals = {}

        def run_kd():
            vals["kid"] = kd.metric_ops(G, D, device)

        def run_pr():
            pr.metric_ops(G, D, device)
            vals["prdc"] = dict(pr.last)
        run_kd(); run_pr()                                                   # warm both
        pr.history.clear()
        t = interleave({"kernel": run_kd, "prdc": run_pr, "kernel#control": run_kd}, a.rounds, device, "metric")
        s = summary(t, host="kernel", dev="prdc", control="kernel#control")
        s["kernel_over_prdc"] = s.pop("host_over_device")
        s.pop("device_not_slower")
        res["metric_ops"] = dict(s, what="KernelDistance.metric_ops against PrecisionRecall.metric_ops, extractor 'discriminator', %d "
                                         "real + %d generated %d^2 images: the per-epoch cost of --kid_samples %d against "
                                         "--pr_samples %d" % (N, N, S, N, N), values=vals)

    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
