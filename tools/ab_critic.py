#!/usr/bin/env python3
"""Interleaved A/B of the benchmarked training iteration with a BatchNorm critic against the BatchNorm-free critic
(DCGANDiscriminator(batchnorm=False)) inside ONE process, with tools/ab_step.py's timing scheme: every workload owns its models,
optimizers, plug-ins and step graphs, the timed regions alternate  bn plain bn#control  (order reversed every other round), and
the BatchNorm workload is built twice -- the difference of the two identically configured copies is the noise floor a delta has
to exceed.  bench.py is used as it stands (bench.hip_workload); the plain workload is built while the package's
DCGANDiscriminator name is bound to the batchnorm=False constructor.

    python tools/ab_critic.py --rounds 5 --steps 20 [--finish-bw] [--json profiles/critic_plain_step.json]

--finish-bw: also time the two slab-finishing kernels (rg_slab_bias_act, rg_slab_mask with column sums) at the two deep-layer
shapes of the benchmark (512 -> 1024 at 16 x 16 and 1024 -> 2048 at 8 x 8, batch 64, both directions) and report achieved
bytes / s next to the stream-copy ceiling rna_gan_amd.probe measures in the same process.
Nothing here is imported by the product or the tests.
"""
import argparse
import functools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402


def build(bench, bargs, device, plain, prime):
    import rna_gan_amd as P
    orig = P.DCGANDiscriminator
    if plain:
        P.DCGANDiscriminator = functools.partial(orig, batchnorm=False)
    try:
        step, flush, _, _ = bench.hip_workload(bargs, 0, 1, device)
    finally:
        P.DCGANDiscriminator = orig
    for _ in range(prime):
        step()
    torch.cuda.synchronize(device)
    return step, flush


def finish_bandwidth(device, batch, precision):
    """Achieved GB/s (bytes read + written) of the finishing kernels on the slabs the deep layers' split-K launches leave."""
    from rna_gan_amd import _abi, probe
    from rna_gan_amd.ops_hip import HipOps
    h16 = torch.float16 if precision == "fp16" else torch.bfloat16
    ops = HipOps(h16, device)
    lib, st = ops.lib, ops.stream
    rows = []
    for I, O, hs in ((512, 1024, 16), (1024, 2048, 8)):
        ho = hs // 2
        for up in (0, 1):
            M, C = (batch * hs * hs, I) if up else (batch * ho * ho, O)
            ns = int(lib.rg_conv_split(up, batch, ho, ho, O, I, ops.dt, ops.algo))
            sdt = int(lib.rg_conv_slab_dtype(up, batch, ho, ho, O, I, ops.dt, ops.algo))
            esz = 4 if sdt == _abi.RG_F32 else 2
            if ns <= 1:
                rows.append({"layer": "%d->%d@%d" % (I, O, hs), "direction": "up" if up else "down", "nsplit": ns})
                continue
            slab = torch.randn(ns * M * C, device=device).to(torch.float32 if esz == 4 else h16)
            bias = torch.randn(C, device=device)
            mask = torch.randn(M, C, device=device).to(h16)
            y = torch.empty(M, C, dtype=h16, device=device)
            prow = int(lib.rg_slab_finish_rows(M, C))
            parts = torch.empty(prow, C, device=device)
            for name, launch, nbytes in (
                    ("rg_slab_bias_act", lambda: _abi.check(lib.rg_slab_bias_act(slab.data_ptr(), ns, M * C, sdt, bias.data_ptr(),
                                                                                 y.data_ptr(), M, C, 0.2, st), "rg_slab_bias_act"),
                     ns * M * C * esz + M * C * 2),
                    ("rg_slab_mask", lambda: _abi.check(lib.rg_slab_mask(slab.data_ptr(), ns, M * C, sdt, mask.data_ptr(), 0.2,
                                                                         y.data_ptr(), parts.data_ptr(), M, C, st), "rg_slab_mask"),
                     ns * M * C * esz + 2 * M * C * 2 + prow * C * 4)):
                ms = probe._timed(launch, 0.3, 32, device)
                rows.append({"layer": "%d->%d@%d" % (I, O, hs), "direction": "up" if up else "down", "kernel": name, "M": M, "C": C,
                             "nsplit": ns, "slab_bytes_per_element": esz, "us": round(ms * 1e3, 2),
                             "gbps": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    ceil = probe.measure_ceilings(device, settle_s=1.0)
    return {"kernels": rows, "stream_copy_gbps": ceil["stream_copy_gbps"], "stream_copy_what": ceil["stream_copy_what"],
            "note": "the slabs of one launch (8-34 MB) fit the 256 MB last-level cache, which the 1 GiB stream copy does not"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prime", type=int, default=40)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--finish-bw", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import bench
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    bargs = bench.parse_args(["--batch", str(a.batch), "--precision", a.precision, "--no-cpu-baseline", "--no-roofline", "--no-extras"])
    names = ["bn", "plain", "bn#control"]
    work, times, last = {}, {n: [] for n in names}, {}
    for n in names:
        t0 = time.perf_counter()
        work[n] = build(bench, bargs, device, n == "plain", a.prime)
        print("[ab_critic] built + primed %-10s in %.1f s" % (n, time.perf_counter() - t0), file=sys.stderr, flush=True)
    for r in range(a.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            step, flush = work[n]
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ls = step()
            flush()
            torch.cuda.synchronize(device)
            times[n].append((time.perf_counter() - t0) / a.steps * 1e3)
            last[n] = [float(x.item()) for x in ls]
        print("[ab_critic] round %d: %s" % (r, "  ".join("%s %.3f" % (n, times[n][-1]) for n in names)), file=sys.stderr, flush=True)
    from rna_gan_amd.ops_hip import check_handoffs
    check_handoffs()
    res = {"what": "ms per training iteration (G-loss, D-loss, penalty train_ops), interleaved in one process", "batch": a.batch,
           "precision": a.precision, "steps": a.steps, "rounds": a.rounds, "variants": []}
    for n in names:
        d = [x - y for x, y in zip(times[n], times["bn"])]
        res["variants"].append({"name": n, "ms": [round(x, 3) for x in times[n]], "mean": round(sum(times[n]) / len(times[n]), 3),
                                "min": round(min(times[n]), 3), "delta_vs_bn": {"mean": round(sum(d) / len(d), 3),
                                                                                "min": round(min(d), 3), "max": round(max(d), 3)},
                                "losses_last_step": [round(x, 5) for x in last[n]]})
    res["noise_floor_ms"] = abs(res["variants"][2]["delta_vs_bn"]["mean"])
    res["plain_minus_bn_ms"] = res["variants"][1]["delta_vs_bn"]["mean"]
    if a.finish_bw:
        del work
        res["finishing_kernels"] = finish_bandwidth(device, a.batch, a.precision)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
