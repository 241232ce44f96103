#!/usr/bin/env python3
"""The kernel-distance evaluation (rna_gan_amd.kid, metrics.KernelDistance) measured on one device, host against device
interleaved in ONE process with the scheme of tools/ab_fd_eval.py: per round every variant is timed once, the order is reversed
every other round, and the host variant is timed twice per round (host, device, host#control) -- the difference of the two
identically configured host timings is the noise floor.

    python tools/ab_kid_eval.py --rows 2048 --features 2048 [--images 2048 --size 256] [--json profiles/kid_device_eval.json]

Sections:
  kernels     rg_polykernel_tile_sums alone at (na, nb, F) = (--rows, --rows, --features), symmetric and two-operand: time and
              fp64 TFLOP/s (2 F flops per computed pair; the symmetric form computes T (T + 1) / 2 of the T^2 tiles), next to the
              nominal 78.6 TFLOP/s and to the rate rg_moments_update reaches in the same process at n = --rows, F = --features
              (the same FMA structure; a rate below half of it means the transposed staging is wrong);
  estimator   kid.mmd2_unbiased on --rows + --rows device features against the host estimator on the same features (numpy fp64
              BLAS Gram matrices, the matrix form of the estimator, on the CPUs the process may use);
  metric      KernelDistance.metric_ops against FrechetDistance.metric_ops with the reference-size networks and --images real
              tiles on the device: the per-epoch cost of --kid_samples next to --fd_samples.
Nothing here is imported by the product or the tests."""
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

from ab_fd_eval import interleave, summary, wall  # noqa: E402

NOMINAL_FP64_TFLOPS = 78.6


def host_mmd2(x, y, gamma=None, coef0=1.0, degree=3):
    """the unbiased estimator from fp64 BLAS Gram matrices (host baseline)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m, n = x.shape[0], y.shape[0]
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    kxx, kyy, kxy = ((gamma * (p @ q.T) + coef0) ** degree for p, q in ((x, x), (y, y), (x, y)))
    return float((kxx.sum() - np.trace(kxx)) / (m * (m - 1.0)) + (kyy.sum() - np.trace(kyy)) / (n * (n - 1.0))
                 - 2.0 * kxy.sum() / (m * float(n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    import rna_gan_amd as P
    from rna_gan_amd import _abi, kid as K, probe
    from rna_gan_amd.metrics import FrechetDistance, KernelDistance
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(0)
    n, Fdim = a.rows, a.features
    res = {"what": "kernel-distance evaluation on one device; host against device interleaved in one process",
           "rows_per_set": n, "features": Fdim, "rounds": a.rounds, "host_threads": torch.get_num_threads(),
           "nominal_fp64_tflops": NOMINAL_FP64_TFLOPS}
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(n, Fdim, generator=gen).to(device)
    y = (torch.randn(n, Fdim, generator=gen) * 1.1 + 0.05).to(device)

    if "kernels" not in skip:
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        T = K._tiles(n)
        sums = torch.zeros(T, T, dtype=torch.float64, device=device)
        diag = torch.zeros(T, dtype=torch.float64, device=device)
        rows = []
        for form, b, d, pairs in (("symmetric", None, diag.data_ptr(), T * (T + 1) // 2 * 4096), ("two-operand", y.data_ptr(), None, T * T * 4096)):
            ms = probe._timed(lambda: _abi.check(lib.rg_polykernel_tile_sums(x.data_ptr(), Fdim, n, b, Fdim, n, Fdim, 1.0 / Fdim, 1.0, 3,
                                                                             sums.data_ptr(), d, st), "polykernel"), 0.3, 16, device)
            rows.append({"kernel": "rg_polykernel_tile_sums", "form": form, "na": n, "nb": n, "F": Fdim, "us": round(ms * 1e3, 1),
                         "fp64_tflops": round(2.0 * pairs * Fdim / (ms * 1e-3) / 1e12, 2)})
        s1 = torch.zeros(Fdim, dtype=torch.float64, device=device)
        s2 = torch.zeros(Fdim, Fdim, dtype=torch.float64, device=device)
        ms = probe._timed(lambda: _abi.check(lib.rg_moments_update(x.data_ptr(), Fdim, n, Fdim, s1.data_ptr(), s2.data_ptr(), st),
                                             "moments"), 0.3, 16, device)
        Tf = K._tiles(Fdim)
        rows.append({"kernel": "rg_moments_update", "n": n, "F": Fdim, "us": round(ms * 1e3, 1),
                     "fp64_tflops": round(2.0 * n * (Tf * (Tf + 1) // 2 * 4096) / (ms * 1e-3) / 1e12, 2)})
        res["kernels"] = rows
        res["polykernel_over_moments_rate"] = round(min(r["fp64_tflops"] for r in rows[:2]) / rows[2]["fp64_tflops"], 2)

    if "estimator" not in skip:
        xh, yh = x.cpu().numpy(), y.cpu().numpy()
        keep = {}

        def host():
            keep["host"] = host_mmd2(xh, yh)

        def dev():
            keep["dev"] = K.mmd2_unbiased(x, y)
        host(); dev()
        t = interleave({"host": host, "device": dev, "host#control": host}, a.rounds, device, "estimator")
        res["estimator"] = dict(summary(t), mmd2_host=keep["host"], mmd2_device=keep["dev"])

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
        kd, fd = KernelDistance(real, batch_size=256, seed=0), FrechetDistance(real, batch_size=256, seed=0)
        vals = {}

        def run_kd():
            vals["kid"] = kd.metric_ops(G, D, device)

        def run_fd():
            vals["fd"] = fd.metric_ops(G, D, device)
        run_kd(); run_fd()                                                   # warm both
        t = interleave({"frechet": run_fd, "kernel": run_kd, "frechet#control": run_fd}, a.rounds, device, "metric")
        res["metric_ops"] = dict(summary(t, host="frechet", dev="kernel", control="frechet#control"),
                                 what="FrechetDistance.metric_ops (named host in the ratio) against KernelDistance.metric_ops, extractor "
                                      "'discriminator', %d real + %d generated %d^2 images: the per-epoch cost of --fd_samples %d "
                                      "against --kid_samples %d" % (N, N, S, N, N), values=vals)

    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
