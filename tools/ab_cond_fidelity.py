#!/usr/bin/env python3
"""The conditioning-fidelity evaluation (rna_gan_amd.representation, metrics.ConditioningFidelity) measured on one device.

    python tools/ab_cond_fidelity.py [--patients 64 --tiles 32 --size 256] [--json profiles/cond_fidelity.json]

Sections:
  kernels     rg_group_sums_update alone at G = 512, F = 2048, n = 4096 (ids r % G) and rg_match_ranks alone at 512 x 512
              centroids of 2048 features: the MEDIAN of --calls single calls, each between two device events, after a warm-up;
  evaluation  one ConditioningFidelity.metric_ops at --patients x --tiles with the reference-size networks (256 x 256, 64 step
              channels, 2048 encoding dims, the 19 198-gene betaVAE) and the discriminator extractor, against the HOST ROUTE in
              the same process: the same tiles synthesised and extracted on the device, then the features downloaded, numpy
              sequential per-patient sums in row order and numpy ranks.  Variants are interleaved (device, host, device#control),
              the order reversed every other round; medians over --rounds.  Both routes must return the same ranks.
Nothing here is imported by the product or the tests."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ab_fd_eval import interleave  # noqa: E402


def median_us(launch, calls, device):
    stream = torch.cuda.current_stream(device)
    for _ in range(5):
        launch()
    torch.cuda.synchronize(device)
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); launch(); e1.record(stream)
        torch.cuda.synchronize(device)
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 1), round(min(out), 1)


def host_route(metric, G, D, device):
    """the evaluation with the reductions on the host: features downloaded, numpy sums in row order, numpy ranks"""
    from rna_gan_amd import fid as FID
    from rna_gan_amd import representation as RP
    modes = [(m, m.training) for m in (G, D)]
    try:
        for m, _ in modes:
            m.eval()
        extract = FID.discriminator_features_device(D)
        with torch.no_grad():
            real = [(extract(RP._real_batch(metric.real_tiles[i:i + metric.batch_size], None, 0.5, 0.5)),
                     metric.patient_of[i:i + metric.batch_size]) for i in range(0, metric.real_tiles.shape[0], metric.batch_size)]
            fake = []
            for patient, z in RP.conditioned_noise(G, metric.betavae, metric.rna, metric.tiles_per_patient, metric.seed, metric.group):
                pos = 0
                for img in RP._generated(G, z.float(), metric.batch_size):
                    fake.append((extract(img), patient[pos:pos + img.shape[0]]))
                    pos += img.shape[0]
        P = metric.rna.shape[0]
        cents = []
        for batches in (fake, real):
            x = torch.cat([f for f, _ in batches]).cpu().numpy()
            ids = torch.cat([i for _, i in batches]).cpu().numpy()
            sums, counts = np.zeros((P, x.shape[1])), np.zeros(P)
            for r in range(x.shape[0]):
                sums[ids[r]] += x[r]
                counts[ids[r]] += 1
            c = sums / counts[:, None]
            cents.append(c - c.mean(axis=0, keepdims=True))
        d = ((cents[0][:, None, :] - cents[1][None, :, :]) ** 2).sum(axis=2)
        ds = np.diagonal(d)[:, None]
        s, t = np.arange(P)[None, :], np.arange(P)[:, None]
        return (((d < ds) & (s != t)).sum(axis=1) + ((d == ds) & (s < t)).sum(axis=1)).astype(np.int32)
    finally:
        for m, was in modes:
            m.train(was)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patients", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--features", type=int, default=19198)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma-separated sections to leave out")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    skip = set(s for s in a.skip.split(",") if s)
    import rna_gan_amd as P
    from rna_gan_amd import _abi, synth
    from rna_gan_amd.metrics import ConditioningFidelity
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"what": "conditioning-fidelity evaluation on one device; medians; host route against device route interleaved in one "
                   "process", "rounds": a.rounds, "calls": a.calls, "host_threads": torch.get_num_threads()}
    if "kernels" not in skip:
        lib = _abi.load()
        st = torch.cuda.current_stream(device).cuda_stream
        Gn, F, n = 512, 2048, 4096
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(n, F, generator=gen).to(device)
        ids = (torch.arange(n, dtype=torch.int32) % Gn).to(device)
        sums = torch.zeros(Gn, F, dtype=torch.float64, device=device)
        counts = torch.zeros(Gn, dtype=torch.int64, device=device)
        med, lo = median_us(lambda: _abi.check(lib.rg_group_sums_update(x.data_ptr(), F, n, F, ids.data_ptr(), Gn, sums.data_ptr(),
                                                                        counts.data_ptr(), st), "group_sums"), a.calls, device)
        rows = [{"kernel": "rg_group_sums_update", "G": Gn, "F": F, "n": n, "median_us": med, "min_us": lo,
                 "read_gb_per_s": round((n * F * 4 + 2 * Gn * F * 8) / (med * 1e-6) / 1e9, 1)}]
        ca = torch.randn(Gn, F, generator=gen, dtype=torch.float64).to(device)
        cb = torch.randn(Gn, F, generator=gen, dtype=torch.float64).to(device)
        rank = torch.empty(Gn, dtype=torch.int32, device=device)
        dt = torch.empty(Gn, dtype=torch.float64, device=device)
        med, lo = median_us(lambda: _abi.check(lib.rg_match_ranks(ca.data_ptr(), F, Gn, cb.data_ptr(), F, Gn, F, None, rank.data_ptr(),
                                                                  dt.data_ptr(), st), "match_ranks"), a.calls, device)
        rows.append({"kernel": "rg_match_ranks", "na": Gn, "nb": Gn, "F": F, "median_us": med, "min_us": lo,
                     "fp64_tflops_useful": round(3.0 * Gn * Gn * F / (med * 1e-6) / 1e12, 2)})
        res["kernels"] = rows
        print(json.dumps(rows), file=sys.stderr, flush=True)
    if "evaluation" not in skip:
        Pn, T, S = a.patients, a.tiles, a.size
        G = synth.seeded_fill_(P.DCGANGenerator(2048, S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.Tanh()), 1).to(device)
        D = synth.seeded_fill_(P.DCGANDiscriminator(S, 3, 64, nonlinearity=nn.LeakyReLU(0.2), last_nonlinearity=nn.LeakyReLU(0.2)), 2).to(device)
        bv = synth.seeded_fill_(P.betaVAE(a.features, 2048, [6000, 4000, 2048], [4000, 6000], beta=0.0005), 3).to(device)
        tiles = synth.synthetic_tiles_u8(Pn * T, S, 4).to(device)
        patient_of = (torch.arange(Pn * T, dtype=torch.int32) % Pn).to(device)
        rna = synth.synthetic_rna(Pn, a.features, 5, distinct=Pn)
        metric = ConditioningFidelity(tiles, patient_of, rna, bv, tiles_per_patient=T, batch_size=256, seed=6)
        ranks = {}

        def dev():
            metric.metric_ops(G, D, device)
            ranks["device"] = metric.last_rank.cpu().numpy()

        def host():
            ranks["host"] = host_route(metric, G, D, device)
        dev(); host()                                            # warm-up of every shape
        times = interleave({"device": dev, "host": host, "device#control": dev}, a.rounds, device, "evaluation")
        out = {k: {"s": [round(v, 4) for v in t], "median": round(statistics.median(t), 4)} for k, t in times.items()}
        out["noise_floor_s"] = round(abs(out["device"]["median"] - out["device#control"]["median"]), 4)
        out["host_over_device"] = round(out["host"]["median"] / out["device"]["median"], 3)
        out["device_not_slower"] = bool(out["device"]["median"] <= out["host"]["median"])
        out["same_ranks"] = bool(np.array_equal(ranks["device"], ranks["host"]))
        out["what"] = ("ConditioningFidelity.metric_ops, extractor 'discriminator', %d patients x %d tiles of %d^2, against the host "
                       "route (same synthesis and features, download, numpy sums and ranks)" % (Pn, T, S))
        out["scores"] = metric.last
        res["evaluation"] = out
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
